/* me_prims_emu.h -- the ME primitives as plain serial C: the bodies the CPU suite's emulation (tests/emu) runs.  Included by me_prims.h
 * only, which lists the names; me_prims_dev.h holds the bodies the kernels run. */
#ifndef SVT_ME_PRIMS_EMU_H
#define SVT_ME_PRIMS_EMU_H
static inline uint64_t svt_qsad(uint64_t ref8, uint32_t src4, uint64_t acc) {
    uint64_t out = 0;
    for (int o = 0; o < 4; o++) {
        uint32_t s = 0;
        for (int b = 0; b < 4; b++) {
            int r = (int)((ref8 >> (8 * (o + b))) & 0xff), c = (int)((src4 >> (8 * b)) & 0xff);
            s += (uint32_t)(r > c ? r - c : c - r);
        }
        out |= (uint64_t)((uint16_t)(((acc >> (16 * o)) & 0xffff) + s)) << (16 * o);
    }
    return out;
}
static inline uint32_t svt_ssd4(uint32_t a, uint32_t b, uint32_t acc) {
    for (int i = 0; i < 4; i++) {
        int d = (int)((a >> (8 * i)) & 0xff) - (int)((b >> (8 * i)) & 0xff);
        acc += (uint32_t)(d * d);
    }
    return acc;
}
static inline uint32_t svt_sad4(uint32_t a, uint32_t b, uint32_t acc) {
    for (int i = 0; i < 4; i++) {
        int x = (int)((a >> (8 * i)) & 0xff), y = (int)((b >> (8 * i)) & 0xff);
        acc += (uint32_t)(x > y ? x - y : y - x);
    }
    return acc;
}
/* per-byte (a + b + 1) >> 1 without carries between bytes */
static inline uint32_t svt_avg4(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7fu); }
static inline uint32_t svt_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3)));
}
static inline void svt_lds_min_u64(uint64_t *p, uint64_t v) { if (v < *p) *p = v; }
static inline void svt_lds_add_u32(uint32_t *p, uint32_t v) { *p += v; }
/* host emulation runs lanes one after the other: a "wave reduction" degenerates to the per-lane update */
static inline void svt_wave_add_u32(uint32_t *p, uint32_t v, int uniform_dst) { (void)uniform_dst; *p += v; }
static inline void svt_wave_min_u64(uint64_t *p, uint64_t v) { if (v < *p) *p = v; }
static inline void svt_group_add_u32(uint32_t *p, uint32_t v, int group) { (void)group; *p += v; }
static inline void svt_group_add_var(uint32_t *p, uint32_t v, int group) { (void)group; *p += v; }
#define ME_MUL(a, b) ((a) * (b))
#define SVT_SCHED_FENCE() ((void)0)
/* per 16-bit lane: min(max(v, 32), 287) - 32 */
static inline uint32_t svt_pk_clamp_sub32(uint32_t v) {
    uint32_t lo = v & 0xffffu, hi = v >> 16;
    lo = (lo < 32 ? 32 : lo > 287 ? 287 : lo) - 32;
    hi = (hi < 32 ? 32 : hi > 287 ? 287 : hi) - 32;
    return lo | (hi << 16);
}
#define SVT_GLOBAL
SVT_DEV uint32_t me_ld32u_g(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
SVT_DEV me_u32x2 me_ld64u_g(const uint8_t *p) { me_u32x2 v; memcpy(&v, p, 8); return v; }
SVT_DEV me_u32x4 me_ld128u_g(const uint8_t *p) { me_u32x4 v; memcpy(&v, p, 16); return v; }
SVT_DEV me_gsrc me_gsrc_of(const uint8_t *p) { me_gsrc g; g.base = p; return g; }
SVT_DEV svt_plane me_plane_uni(const svt_plane *p) { return *p; }
SVT_DEV int me_udiv(int t, int d) { return t / d; }
/* 4-tap {-2,18,18,-2} (+16)>>5 with clipping on 4 packed samples: a,b,d,e hold the 4 taps of 4 neighbouring
 * outputs.  Even and odd bytes are processed as two 16-bit lanes of one register; a bias of 1024 (= 32 << 5) keeps
 * every lane non-negative so nothing borrows across lanes: floor((S + 1024) / 32) = floor(S / 32) + 32. */
SVT_DEV uint32_t me_tap4_half(uint32_t a, uint32_t b, uint32_t d, uint32_t e) {
    const uint32_t s2 = (b + d) << 1;                          /* 18 x = 16 x + 2 x */
    uint32_t       v = (s2 << 3) + s2 + 0x04100410u - ((a + e) << 1); /* per lane: 18(b+d) + 16 + 1024 - 2(a+e) in [20, 10220] */
    v = (v >> 5) & 0x07ff07ffu;
    return svt_pk_clamp_sub32(v); /* per lane: min(max(v, 32), 287) - 32 */
}
SVT_DEV uint32_t me_tap4_x4(uint32_t a, uint32_t b, uint32_t d, uint32_t e) {
    const uint32_t M = 0x00ff00ffu;
    uint32_t ev = me_tap4_half(a & M, b & M, d & M, e & M);
    uint32_t od = me_tap4_half((a >> 8) & M, (b >> 8) & M, (d >> 8) & M, (e >> 8) & M);
    return ev | (od << 8);
}
SVT_DEV uint32_t me_pair16(uint32_t hi, uint32_t lo, int k) { /* bytes k and k + 2 of the 8-byte pair, zero-extended into the two 16-bit lanes */
    const uint64_t v = ((uint64_t)hi << 32) | lo;
    return (uint32_t)((v >> (8 * k)) & 0xff) | ((uint32_t)((v >> (8 * (k + 2))) & 0xff) << 16);
}
SVT_DEV uint32_t me_half_lanes(uint32_t r) { return r; }
SVT_DEV uint32_t me_half_join(uint32_t ev, uint32_t od) {
    return (ev & 0xffu) | ((od & 0xffu) << 8) | (((ev >> 16) & 0xffu) << 16) | (((od >> 16) & 0xffu) << 24);
}
/* list 0's prediction dwords of the bi-pred lanes wait in memory: ME_PR(j) = pred0[j * 256 + tid] (me_layout.h reserves the bytes) */
#define ME_PR(j) pr[(j) * SVT_NT]
#define ME_PRED0_DECL() ((void)0)
#define ME_PRED0_REGS (c->pred0 + tid)
/* a phase runs its 256 lanes one after the other; a barrier is the end of that loop */
#define ME_PHASE(...) do { for (int tid = 0; tid < SVT_NT; tid++) { __VA_ARGS__; } } while (0)
#define ME_UNIFORM_WRITE(...) do { __VA_ARGS__; } while (0)
#define ME_UNI(x) ((int)(x)) /* (nothing to move to a scalar register) */
#define ME_PLAN_RD(x) (x)
/* tasks outside a phase: the one call (tid 0) walks them all */
#define ME_TASKS(t, n) for (int t = 0; t < (n); t++)
SVT_DEV uint32_t me_magic_small(int d) { return me_magic_of(d); }
SVT_DEV void svt_wave_min_key32(uint64_t *p, uint32_t k) { if (k != 0xffffffffu && me_hme_key64(k) < *p) *p = me_hme_key64(k); }
/* no clock here: me_prof.h makes every mark a no-op */
#define ME_PROF_OFF 1
#endif
