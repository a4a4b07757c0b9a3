/* me_prims.h -- what the ME phases are written in.  Every name below has two bodies: me_prims_dev.h (hipcc: builtins, DPP, LDS atomics,
 * scalar-register moves) and me_prims_emu.h (a host compiler with -DSVT_HOST_EMU: plain C, lanes one after the other).  The conditional
 * below is the only place that chooses between them; one on SVT_HOST_EMU anywhere else marks a device-only phase variant.
 *   qualifiers  SVT_GLOBAL (SVT_DEV is chosen below, with the file of bodies)
 *   arithmetic  svt_qsad svt_sad4 svt_ssd4 svt_avg4 svt_alignbyte svt_pk_clamp_sub32 ME_MUL me_udiv me_magic_small
 *               me_tap4_half me_tap4_x4 me_pair16 me_half_lanes me_half_join
 *   memory      me_ld32u_g me_ld64u_g me_ld128u_g me_gsrc_of me_plane_uni
 *   reductions  svt_lds_min_u64 svt_lds_add_u32 svt_wave_add_u32 svt_wave_min_u64 svt_wave_min_key32 svt_group_add_u32 svt_group_add_var
 *   control     ME_PHASE ME_UNIFORM_WRITE ME_UNI ME_PLAN_RD ME_TASKS SVT_SCHED_FENCE ME_PR ME_PRED0_DECL ME_PRED0_REGS
 * Device only, for the device-only variants and the other kernels of me_kernel.hip: SVT_DPP_ADD svt_row_prefix_add
 * svt_wave_add_u32_to_lane0 me_tap4_join me_magics.  Emulation only: ME_PROF_OFF (me_prof.h). */
#ifndef SVT_ME_PRIMS_H
#define SVT_ME_PRIMS_H
#include <stdint.h>
#include <string.h>
#include "../../include/svtvp9_hip.h"
#ifdef SVT_HOST_EMU
#define SVT_DEV static inline
#define ME_PRIMS_BODIES "me_prims_emu.h"
#else
#include <hip/hip_runtime.h>
#define SVT_DEV __device__ __forceinline__
#define ME_PRIMS_BODIES "me_prims_dev.h"
#endif
#define SVT_NT 256

/* ---- plain helpers the pairs lean on ---- */
/* 8 / 16 bytes from a global byte address of any alignment: one global_load_dwordx2 / x4 */
typedef struct me_u32x2 { uint32_t x, y; } me_u32x2;
typedef struct me_u32x4 { uint32_t x, y, z, w; } me_u32x4;
/* A rectangle of global memory addressed as one uniform base (scalar registers -> the loads use the scalar-base addressing
 * form with a 32-bit lane offset, no 64-bit address arithmetic per lane) plus byte offsets. */
typedef struct me_gsrc { const uint8_t *base; } me_gsrc;
#define SVT_AS_GLOBAL(T, p) ((T SVT_GLOBAL *)(uintptr_t)(p))
/* t / d through inv = floor((2^32 - 1) / d) + 1 (exact while t * d < 2^32; d = 1 gives inv = 0 -> t).  Every thread derives
 * inv itself when it enters a window: the (slow) division runs in parallel instead of on the planning thread */
SVT_DEV uint32_t me_magic_of(int d) { return (uint32_t)(0xffffffffu / (uint32_t)d) + 1u; }
/* 32-bit form of the HME key for the 1/16-resolution level: (sad << 16) | (y << 8) | x -- the SAD of a 16 x 8 block is below
 * 2^15 and the search positions of a region stay below 256 either way; ordered exactly like the 64-bit key it stands for */
SVT_DEV uint64_t me_hme_key64(uint32_t k) { return ((uint64_t)(k >> 16) << 32) | (((k >> 8) & 0xffu) << 16) | (k & 0xffu); }

#include ME_PRIMS_BODIES

/* ---- one body for both, built on the pairs ---- */
/* unaligned 32-bit fetch from a byte address (LDS or global): two aligned loads + v_alignbyte.  Branch-free on
 * purpose: a conditional second load serialises the two memory round trips and keeps the compiler from batching the
 * loads of unrolled callers.  An aligned address re-reads its own dword, so nothing beyond the 4 bytes is touched. */
SVT_DEV uint32_t me_ld32u(const uint8_t *p) {
    const uint32_t  sh = (uint32_t)((uintptr_t)p & 3);
    const uint32_t *q  = (const uint32_t *)(p - sh);
    const uint32_t  lo = q[0], hi = q[sh ? 1 : 0];
    return svt_alignbyte(hi, lo, sh);
}
/* the 4 bytes at byte offset off of the rectangle */
SVT_DEV uint32_t me_gld(const me_gsrc g, uint32_t off) { return me_ld32u_g(g.base + off); }
SVT_DEV int me_div_magic(int t, uint32_t inv) { return inv ? (int)(((uint64_t)(uint32_t)t * inv) >> 32) : t; }
#endif
