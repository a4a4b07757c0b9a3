/* me_prims_dev.h -- the ME primitives as gfx950 builtins, DPP reductions, LDS atomics and address-space casts: the bodies the kernels run.
 * Included by me_prims.h only, which lists the names; me_prims_emu.h holds the serial C bodies of the CPU suite's emulation. */
#ifndef SVT_ME_PRIMS_DEV_H
#define SVT_ME_PRIMS_DEV_H
SVT_DEV uint64_t svt_qsad(uint64_t ref8, uint32_t src4, uint64_t acc) {
    return __builtin_amdgcn_qsad_pk_u16_u8(ref8, src4, acc);
}
SVT_DEV uint32_t svt_sad4(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_sad_u8(a, b, acc); }
/* sum of squared differences of 4 packed samples: a.a + b.b - 2 a.b with three v_dot4_u32_u8 */
SVT_DEV uint32_t svt_ssd4(uint32_t a, uint32_t b, uint32_t acc) {
    acc = __builtin_amdgcn_udot4(a, a, acc, false);
    acc = __builtin_amdgcn_udot4(b, b, acc, false);
    return acc - 2u * __builtin_amdgcn_udot4(a, b, 0u, false);
}
SVT_DEV uint32_t svt_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
/* per-byte (a + b + 1) >> 1: v_lerp_u8 with the rounding bit set in every byte of the third operand */
SVT_DEV uint32_t svt_avg4(uint32_t a, uint32_t b) { return __builtin_amdgcn_lerp(a, b, 0x01010101u); }
/* per 16-bit lane: min(max(v, 32), 287) - 32 (v_pk_max_u16 / v_pk_min_u16 / v_pk_sub_u16) */
typedef unsigned short svt_u16x2 __attribute__((ext_vector_type(2)));
SVT_DEV uint32_t svt_pk_clamp_sub32(uint32_t v) {
    svt_u16x2 x = __builtin_bit_cast(svt_u16x2, v);
    const svt_u16x2 lo = {32, 32}, hi = {287, 287};
    x = __builtin_elementwise_min(__builtin_elementwise_max(x, lo), hi) - lo;
    return __builtin_bit_cast(uint32_t, x);
}
/* keeps the instruction scheduler from interleaving unrolled iterations (and their live registers) */
#define SVT_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
SVT_DEV void svt_lds_min_u64(uint64_t *p, uint64_t v) { /* lanes of one instruction must target different addresses */
    __hip_atomic_fetch_min((unsigned long long *)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
SVT_DEV void svt_lds_add_u32(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
/* products of small offsets (rows, strides: far below 2^23): full-rate 24-bit multiply instead of v_mul_lo_u32 */
#define ME_MUL(a, b) __mul24((int)(a), (int)(b))
/* Cross-lane reductions use DPP row shifts (a few cycles each) instead of ds_bpermute shuffles (~90 cycles each,
 * measured), and never let several lanes of one instruction hit the same LDS address with an atomic (~100 cycles
 * per lane, measured with tools/ubench_me.hip). */
#define SVT_DPP_ADD(v, ctrl) ((v) + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), 0xf, 0xf, true))
/* inclusive prefix sum inside each row of 16 lanes, up to `span` lanes back (span = 4, 8 or 16) */
SVT_DEV uint32_t svt_row_prefix_add(uint32_t v, int span) {
    v = SVT_DPP_ADD(v, 0x111); /* row_shr:1 */
    v = SVT_DPP_ADD(v, 0x112); /* row_shr:2 */
    if (span >= 8) v = SVT_DPP_ADD(v, 0x114);
    if (span >= 16) v = SVT_DPP_ADD(v, 0x118);
    return v;
}
/* sum over the 64 lanes of the wave (all lanes must call; inactive contributions pass 0) then ONE LDS atomic */
SVT_DEV void svt_wave_add_u32(uint32_t *p, uint32_t v, int uniform_dst) {
    (void)uniform_dst;
    v = svt_row_prefix_add(v, 16);
    const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)v, 15) + (uint32_t)__builtin_amdgcn_readlane((int)v, 31) +
                       (uint32_t)__builtin_amdgcn_readlane((int)v, 47) + (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(p, t);
}
/* sum over the wave, result in every lane's *v (all lanes must call) */
SVT_DEV void svt_wave_add_u32_to_lane0(uint32_t *v) {
    uint32_t x = svt_row_prefix_add(*v, 16);
    *v = (uint32_t)__builtin_amdgcn_readlane((int)x, 15) + (uint32_t)__builtin_amdgcn_readlane((int)x, 31) +
         (uint32_t)__builtin_amdgcn_readlane((int)x, 47) + (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
/* min over the wave of 64-bit keys (all lanes must call; pass ~0 for "nothing"), then ONE LDS atomic */
SVT_DEV void svt_wave_min_u64(uint64_t *p, uint64_t v) {
#define SVT_DPP_MIN64(ctrl) do { \
        const uint32_t oh_ = (uint32_t)__builtin_amdgcn_update_dpp((int)(v >> 32), (int)(v >> 32), (ctrl), 0xf, 0xf, false); \
        const uint32_t ol_ = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)v, (int)(uint32_t)v, (ctrl), 0xf, 0xf, false); \
        const uint64_t w_ = ((uint64_t)oh_ << 32) | ol_; v = w_ < v ? w_ : v; } while (0)
    SVT_DPP_MIN64(0x111); SVT_DPP_MIN64(0x112); SVT_DPP_MIN64(0x114); SVT_DPP_MIN64(0x118);
#undef SVT_DPP_MIN64
    uint64_t m = ~0ull;
    _Pragma("unroll") for (int l = 15; l < 64; l += 16) {
        const uint64_t w = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
        m = w < m ? w : m;
    }
    if ((threadIdx.x & 63) == 0 && m != ~0ull) __hip_atomic_fetch_min((unsigned long long *)p, (unsigned long long)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
/* sum over aligned groups of `group` (4, 8, 16 or 64) consecutive lanes that share one destination; whole groups are
 * active or inactive together.  The last lane of the group holds the sum and issues the LDS add. */
SVT_DEV void svt_group_add_u32(uint32_t *p, uint32_t v, int group) {
    v = svt_row_prefix_add(v, group);
    if (group == 64)
        v = (uint32_t)__builtin_amdgcn_readlane((int)v, 15) + (uint32_t)__builtin_amdgcn_readlane((int)v, 31) +
            (uint32_t)__builtin_amdgcn_readlane((int)v, 47) + (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    if ((threadIdx.x & (group - 1)) == (unsigned)(group - 1) && v) atomicAdd(p, v);
}
/* as svt_group_add_u32, but the group size (1, 2, 4, 8 or 16 consecutive lanes, aligned) may differ from lane to lane inside a
 * wave: every lane runs the four row-shift steps and picks the partial sum that covers its own group */
SVT_DEV void svt_group_add_var(uint32_t *p, uint32_t v, int group) {
    const uint32_t s1 = SVT_DPP_ADD(v, 0x111);
    const uint32_t s2 = SVT_DPP_ADD(s1, 0x112); /* 4 lanes */
    const uint32_t s3 = SVT_DPP_ADD(s2, 0x114);
    const uint32_t s4 = SVT_DPP_ADD(s3, 0x118); /* 16 lanes */
    const uint32_t t = group == 1 ? v : group == 2 ? s1 : group == 4 ? s2 : group == 8 ? s3 : s4;
    if ((threadIdx.x & (group - 1)) == (unsigned)(group - 1) && t) atomicAdd(p, t);
}
/* Pointers into picture planes and result arrays are known to be global memory: saying so turns the generic
 * (flat_load: 64-bit address per lane, aperture check, counted against the LDS counter too) accesses into global_load /
 * global_store, which also accept a scalar base plus a 32-bit lane offset. */
#define SVT_GLOBAL __attribute__((address_space(1)))
/* 32 bits from a global byte address of any alignment: ONE load.  Global (and scratch) accesses need no alignment on this
 * target (the compiler emits a single global_load_dword for an align-1 dword; the texture unit splits the rare access that
 * straddles a line) -- only LDS penalises misalignment, which is why me_ld32u below still assembles its dword from two. */
typedef uint32_t __attribute__((aligned(1))) me_u32_unaligned;
SVT_DEV uint32_t me_ld32u_g(const uint8_t *p) { return *SVT_AS_GLOBAL(const me_u32_unaligned, p); }
typedef uint32_t me_v2u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t me_v4u __attribute__((ext_vector_type(4), aligned(1)));
SVT_DEV me_u32x2 me_ld64u_g(const uint8_t *p) { const me_v2u t = *SVT_AS_GLOBAL(const me_v2u, p); me_u32x2 v = {t.x, t.y}; return v; }
SVT_DEV me_u32x4 me_ld128u_g(const uint8_t *p) { const me_v4u t = *SVT_AS_GLOBAL(const me_v4u, p); me_u32x4 v = {t.x, t.y, t.z, t.w}; return v; }
SVT_DEV me_gsrc me_gsrc_of(const uint8_t *p) {
    me_gsrc   g;
    uintptr_t a = (uintptr_t)p;
    a  = ((uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    g.base = (const uint8_t *)a;
    return g;
}
/* a plane descriptor read from LDS (or HBM) into scalar registers: every lane holds the same values, and with them in
 * SGPRs the address arithmetic built on them (clipping, me_pix, row offsets) runs on the scalar unit */
SVT_DEV svt_plane me_plane_uni(const svt_plane *p) {
    svt_plane u;
    const uintptr_t a = (uintptr_t)p->buf;
    u.buf = (const uint8_t *)(((uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)) << 32) |
                              (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a));
    u.stride = __builtin_amdgcn_readfirstlane(p->stride); u.origin_x = __builtin_amdgcn_readfirstlane(p->origin_x);
    u.origin_y = __builtin_amdgcn_readfirstlane(p->origin_y); u.width = __builtin_amdgcn_readfirstlane(p->width);
    u.height = __builtin_amdgcn_readfirstlane(p->height);
    return u;
}
/* t / d for a small wave-uniform divisor d (phase geometry: units per row, lanes per strip, search width ...).  An integer
 * division costs ~25 vector instructions per wave here; the reciprocals of 1..256 sit in constant memory instead (one scalar
 * load) and the quotient is one v_mul_hi: exact while t * d < 2^32 (inv = floor((2^32 - 1) / d) + 1; d = 1 -> inv = 0 -> t). */
struct me_magic_table {
    uint32_t v[257];
    constexpr me_magic_table() : v() { for (uint32_t d = 1; d <= 256; d++) v[d] = (uint32_t)(0xffffffffu / d) + 1u; }
};
__constant__ const me_magic_table me_magics = me_magic_table();
SVT_DEV int me_udiv(int t, int d) {
    const int du = __builtin_amdgcn_readfirstlane(d);
    if (du > 256) return t / du;
    const uint32_t inv = me_magics.v[du];
    return inv ? (int)__umulhi((uint32_t)t, inv) : t;
}
/* 4-tap {-2,18,18,-2} (+16)>>5 with clipping on 4 packed samples: a,b,d,e hold the 4 taps of 4 neighbouring
 * outputs.  Even and odd bytes are processed as two 16-bit lanes of one register; a bias of 1024 (= 32 << 5) keeps
 * every lane non-negative so nothing borrows across lanes: floor((S + 1024) / 32) = floor(S / 32) + 32. */
SVT_DEV uint32_t me_tap4_half(uint32_t a, uint32_t b, uint32_t d, uint32_t e) {
    /* on the packed 16-bit ALU, signed: two adds, two multiply-adds, an arithmetic shift; v_sat_pk_u8_i16 is the clip and
     * leaves the two samples in bytes 0 and 1 */
    typedef short   s16x2 __attribute__((ext_vector_type(2)));
    const s16x2     A = __builtin_bit_cast(s16x2, a), B = __builtin_bit_cast(s16x2, b), D = __builtin_bit_cast(s16x2, d), E = __builtin_bit_cast(s16x2, e);
    const s16x2     k5 = {5, 5};
    /* 18 (b + d) + 16, then - 2 (a + e) on top: two v_pk_mad_i16 (the compiler splits them into mul / shift / sub / add);
     * the value stays in [-1004, 9196] */
    uint32_t        m;
    __asm__("v_pk_mad_i16 %0, %1, 18, 16 op_sel_hi:[1,0,0]" : "=v"(m) : "v"(__builtin_bit_cast(uint32_t, B + D)));
    __asm__("v_pk_mad_i16 %0, %1, -2, %2 op_sel_hi:[1,0,1]" : "=v"(m) : "v"(__builtin_bit_cast(uint32_t, A + E)), "v"(m));
    s16x2           v = __builtin_bit_cast(s16x2, m) >> k5;
    uint32_t r;
    __asm__("v_sat_pk_u8_i16 %0, %1" : "=v"(r) : "v"(__builtin_bit_cast(uint32_t, v)));
    return r;
}
/* even samples in bytes 0,1 of ev, odd ones in bytes 0,1 of od -> the 4 samples in order */
SVT_DEV uint32_t me_tap4_join(uint32_t ev, uint32_t od) { return __builtin_amdgcn_perm(od, ev, 0x05010400u); }
SVT_DEV uint32_t me_tap4_x4(uint32_t a, uint32_t b, uint32_t d, uint32_t e) {
    /* even / odd bytes zero-extended into the two 16-bit lanes with one v_perm_b32 each (selector 0x0c = constant 0) */
    const uint32_t SE = 0x0c020c00u, SO = 0x0c030c01u;
    const uint32_t ev = me_tap4_half(__builtin_amdgcn_perm(0, a, SE), __builtin_amdgcn_perm(0, b, SE), __builtin_amdgcn_perm(0, d, SE), __builtin_amdgcn_perm(0, e, SE));
    const uint32_t od = me_tap4_half(__builtin_amdgcn_perm(0, a, SO), __builtin_amdgcn_perm(0, b, SO), __builtin_amdgcn_perm(0, d, SO), __builtin_amdgcn_perm(0, e, SO));
    return me_tap4_join(ev, od);
}
SVT_DEV uint32_t me_pair16(uint32_t hi, uint32_t lo, int k) { /* bytes k and k + 2 of the 8-byte pair, zero-extended into the two 16-bit lanes */
    return __builtin_amdgcn_perm(hi, lo, 0x0c000c00u | (uint32_t)k | ((uint32_t)(k + 2) << 16));
}
SVT_DEV uint32_t me_half_lanes(uint32_t r) { /* result of me_tap4_half -> its two samples in the two 16-bit lanes */
    return __builtin_amdgcn_perm(0, r, 0x0c010c00u);
}
SVT_DEV uint32_t me_half_join(uint32_t ev, uint32_t od) { /* even / odd results of me_tap4_half -> the four samples in order */
    return me_tap4_join(ev, od);
}
typedef uint64_t __attribute__((aligned(4))) me_u64a4; /* a dword pair in LDS: ds_read2_b32 */
/* list 0's prediction dwords of the bi-pred lanes wait in the lane's own registers (ph_store_pred0) */
#define ME_PR(j) pr[(j)]
#define ME_PRED0_DECL() uint32_t pred0_regs[16]
#define ME_PRED0_REGS pred0_regs
/* the thread index is re-read through an opaque move at every phase: whatever a phase derives from it (lane roles,
 * LDS addresses) is computed where it is used and dies with the phase, instead of being hoisted to the top of the
 * kernel and kept (or spilled) across all the others */
#define ME_PHASE(...) do { __asm__ volatile("" : "+v"(tid)); __VA_ARGS__; __syncthreads(); } while (0)
/* uniform state written to LDS by one thread, followed by a barrier */
#define ME_UNIFORM_WRITE(...) do { if (tid == 0) { __VA_ARGS__; } __syncthreads(); } while (0)
/* a value every lane holds identically (read from LDS): move it to a scalar register */
#define ME_UNI(x) __builtin_amdgcn_readfirstlane((int)(x))
/* a value the planning thread (alone in its wave) reads from LDS: on the device it goes to a scalar register, so that the
 * arithmetic built on it -- placement, clipping, window sizes: everything a level's plan computes -- runs on the scalar unit
 * instead of as a chain of dependent vector instructions of one lane (the workgroup waits for this thread: with the one or two
 * waves per SIMD the 64x64-area configurations leave, its latency is not hidden by anything) */
#define ME_PLAN_RD(x) __builtin_amdgcn_readfirstlane((int)(x))
/* tasks outside a phase: strided over the workgroup's lanes */
#define ME_TASKS(t, n) for (int t = tid; t < (n); t += SVT_NT)
/* (d is the same in every active lane -- the planning thread is alone: a scalar load through the constant cache instead of a vector
 * load with its ~1 us round trip on the critical path of the workgroup) */
SVT_DEV uint32_t me_magic_small(int d) { const int du = __builtin_amdgcn_readfirstlane(d); return du <= 256 ? me_magics.v[du] : me_magic_of(du); }
/* min over the wave (all lanes must call; ~0 = nothing), then ONE 64-bit LDS atomic by lane 0 */
SVT_DEV void svt_wave_min_key32(uint64_t *p, uint32_t k) {
#define SVT_DPP_MIN32(ctrl) do { const uint32_t o_ = (uint32_t)__builtin_amdgcn_update_dpp((int)k, (int)k, (ctrl), 0xf, 0xf, false); k = o_ < k ? o_ : k; } while (0)
    SVT_DPP_MIN32(0x111); SVT_DPP_MIN32(0x112); SVT_DPP_MIN32(0x114); SVT_DPP_MIN32(0x118);
#undef SVT_DPP_MIN32
    uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)k, 15);
    _Pragma("unroll") for (int l = 31; l < 64; l += 16) { const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)k, l); m = w < m ? w : m; }
    if ((threadIdx.x & 63) == 0 && m != 0xffffffffu)
        __hip_atomic_fetch_min((unsigned long long *)p, (unsigned long long)me_hme_key64(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
#endif
