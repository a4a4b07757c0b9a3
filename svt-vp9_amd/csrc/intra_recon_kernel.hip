/*
 * intra_recon_kernel.hip -- the DECODE pass of an intra picture's blocks (gfx950): reference samples, the ten VP9 predictors, then
 * dequantisation / inverse transform / reconstruction of every block from its quantised coefficients and eob, in the dependency order
 * intra prediction imposes.  The coefficient-driven twin of svt_intra_kernel (intra_kernel.hip): what that kernel does with the
 * source in hand (tq_block_body: forward transform, quantiser, inverse) this one does from what a frame reader returned
 * (rc_block_body, rc_core.h: the body svt_rc_kernel runs for inter pictures) -- the reconstruction process of the VP9 specification for
 * intra blocks, i.e. the prediction of VPX/vp9_reconintra.c:249-408 followed by eb_vp9_idct*_add / eb_vp9_iht*_add (VPX/vp9_idct.c:111-189).
 *
 * THE WALK IS svt_intra_kernel's, RULE FOR RULE (its file and kernel comments give the reasons; none is repeated here): 256-thread
 * workgroups of four independent 64-lane workers that never meet (no workgroup barrier anywhere), tickets drawn by lane 0 behind a
 * tq_block_sync and broadcast with readfirstlane, svt_intra_cell_of_ticket's anti-diagonal order over 16x16 luma cells times three planes,
 * the waits at the left and above cells' flags (for a 32x32 block: its lowest left and its rightmost above neighbour), a 32x32 block coded
 * by the ticket of its top-right cell, which sets four flags, inter leaves skipped in a `mixed` picture, the block's stores written through
 * and read back with agent-scope accesses (no release / acquire fences), drained with s_waitcnt vmcnt(0) before the relaxed flag store.
 * Which cells are coded and that every drawn ticket that passes the 32x32 rule publishes its flag depends on the mode-info grid alone:
 * coefficients and eobs are never looked at by the walk, so a picture terminates whatever the coefficient arrays hold.  A malformed unit sets
 * the status bit and its cell still publishes.
 *
 * The above-right rule is the ENCODE pass's (have_right = 0 for blocks >= 8x8; a 4x4 block in the left half of its unit reads four
 * above-right samples): this kernel rebuilds what svt_intra_kernel reconstructed.
 *
 * Outputs: the prediction (optional), the reconstruction, nz[unit] = 1 where a block of the unit has a non-zero eob; the eob map and the
 * coefficients are inputs and are not written.  Coefficients whose dequantised product leaves 16 bits (counted as svt_rc_kernel counts
 * them, of blocks with eob != 0) are summed per worker in a register and added to *overflow once, when the worker's tickets run out.
 */
#include <hip/hip_runtime.h>
#include "tq_core.h"
#include "rc_core.h"
#include "encdec_core.h"
#include "intra_pred.h"
#include "intra_core.h"
#include "wave_ops.h"
#include <stdlib.h>

#ifdef INTRA_FENCES
#error "svt_intra_rc_kernel has no fence form: its stores are written through and its reference samples read with agent-scope loads"
#endif

namespace {

/* one N x N transform block of plane `plane` at sample (x0, y0) of that plane; the whole worker (one wave) calls it.  lds: the
 * workgroup's LDS; the worker's slice is derived here, per block (intra_block's reason).  Of P, src / dqcoeff / iscan are not looked at and
 * qcoeff / eob_map are only read.  Returns the block's eob (uniform); ovf: += the lane's coefficients that overflowed 16 bits. */
template <int N>
__device__ __forceinline__ int intra_rc_block(const intra_pic_dev &P, int plane, int x0, int y0, int mode, int sb, int32_t *lds, uint32_t &ovf, int have_right = 0) {
    const int lane = (int)__lane_id(), c = plane ? 1 : 0;
    int32_t *const tile = lds + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) * INTRA_SLICE_DW;
    uint8_t *const edge = (uint8_t *)(tile + INTRA_TILE_DW);
    const int rs = P.rec_stride[c];
    uint8_t  *rp = P.rec[plane];
    const int have_left = x0 > 0, have_top = y0 > 0;
    const bool active = lane < N;
    const int  i = lane % N;
    uint32_t   prow[N / 4], qrow[N / 2];
    constexpr uintptr_t AM = N >= 16 ? 15 : N - 1;
    /* the block's eob and its coefficient row do not depend on the neighbours: their loads are issued first and complete under the
       reference-sample loads */
    const int pw4 = (plane ? P.width >> 1 : P.width) >> 2, w4 = P.width >> 2, h4 = P.height >> 2;
    const int eo = plane == 0 ? 0 : w4 * h4 + (plane == 2 ? (w4 >> 1) * (h4 >> 1) : 0);
    const int eob = __builtin_amdgcn_readfirstlane((int)P.eob_map[eo + (y0 >> 2) * pw4 + (x0 >> 2)]);
    const uint32_t coeff_off = (uint32_t)sb * SVT_SB_COEFFS + (plane == 0 ? 0u : plane == 1 ? 4096u : 5120u) + svt_zorder4((x0 & (plane ? 31 : 63)) >> 2, (y0 & (plane ? 31 : 63)) >> 2) * 16u;
    _Pragma("unroll") for (int q = 0; q < N / 2; q++) qrow[q] = 0u;
    if (active && eob) { /* row i of the coefficients: 2 N bytes per lane, consecutive lanes consecutive rows */
        const int16_t *qp = P.qcoeff + coeff_off + i * N;
        if constexpr (N == 4) { const uint2 w = *(const uint2 *)qp; qrow[0] = w.x; qrow[1] = w.y; }
        else {
            _Pragma("unroll") for (int j = 0; j < N / 8; j++) {
                const uint4 w = ((const uint4 *)qp)[j];
                qrow[4 * j] = w.x; qrow[4 * j + 1] = w.y; qrow[4 * j + 2] = w.z; qrow[4 * j + 3] = w.w;
            }
        }
    }
    /* reference samples -> LDS (generate_intra_reference_samples, the paths of a block inside the picture): intra_block's text */
    {
        const int j = lane & 31;
        if (lane < 32) { /* left column */
            if (j < N) edge[32 - (j + 1)] = have_left ? INTRA_LD(&rp[(size_t)(y0 + j) * rs + x0 - 1]) : (uint8_t)129;
        } else {         /* above row, replicated to the right */
            if (j < N) {
                const uint8_t a = have_top ? INTRA_LD(&rp[(size_t)(y0 - 1) * rs + x0 + j]) : (uint8_t)127;
                edge[32 + 1 + j] = a;
                /* the right half of the row: true above-right samples for a 4x4 luma block in the left half of its unit (have_right,
                   EbEncDecProcess.c:1146, 1279-1288), copies of the last sample otherwise */
                if (N == 4 && have_right) edge[32 + 1 + N + j] = have_top ? INTRA_LD(&rp[(size_t)(y0 - 1) * rs + x0 + N + j]) : (uint8_t)127;
                else if (j == N - 1) { _Pragma("unroll") for (int q = 0; q < N; q++) edge[32 + 1 + N + q] = a; }
            }
        }
        if (lane == 0) edge[32] = have_top ? (have_left ? INTRA_LD(&rp[(size_t)(y0 - 1) * rs + x0 - 1]) : (uint8_t)129) : (uint8_t)127;
    }
    tq_block_sync(); /* edge[] is written and read by this wave alone */
    intra_pred_row<N>(edge, mode, i, have_left, have_top, prow);
    {
        if (active && P.pred[plane]) {
            uint8_t *pp = P.pred[plane] + (size_t)(y0 + i) * P.pred_stride[c] + x0;
            row_store<N>(pp, ((uintptr_t)pp & AM) == 0, prow);
        }
    }
    svt_tq_block k;
    k.src_off = k.pred_off = 0;
    k.recon_off = (uint32_t)y0 * (uint32_t)rs + (uint32_t)x0;
    k.coeff_off = coeff_off;
    k.tx_size = (uint8_t)txcfg<N>::size;
    k.tx_type = (uint8_t)((plane == 0 && N < 32) ? intra_tx_type(mode) : 0);
    k.iscan_off = P.iscan_off[k.tx_size * 4 + k.tx_type];
    k.src_stride = k.pred_stride = 0; k.recon_stride = (uint16_t)rs;
    k.qtab = (uint8_t)c; k.do_recon = 1; k.partial32 = 0; k.pad_[0] = 0;
    int32_t *t = tile + (lane / N) * (N * (N + 1)); /* the idle slots of the wave run along on tiles of their own (their coefficients read 0) */
    const uint32_t dqp = ((const uint32_t *)(P.qtabs + c))[4]; /* dequant[0], dequant[1]: the fifth dword of the 20-byte table */
    ovf += rc_block_body<N, true>(k, active, i, t, prow, qrow, dqp, eob, rp);
    /* the block's reconstruction is read by the next block of this wave: drain the stores */
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    tq_block_sync();
    return eob;
}

/* Register budget and packing: svt_intra_kernel's (128 VGPRs, four workers per workgroup, INTRA_SLICE_DW dwords of LDS each), so that
 * beside the motion-estimation instance this pass costs a CU no more than the encode form does.  No workgroup barrier: the workers of a
 * workgroup draw different tickets and leave at different moments.  Deadlock freedom: a worker waits only at flags of smaller tickets. */
__global__ __launch_bounds__(64 * INTRA_W) __attribute__((amdgpu_waves_per_eu(4, 4))) void svt_intra_rc_kernel(const intra_pic_dev P, const int n_workers, uint32_t *overflow) {
    constexpr int W = INTRA_W;
    __shared__ int32_t s_lds[W * INTRA_SLICE_DW];
    /* the worker: wave-uniform, and known to be so (readfirstlane) -- it selects the LDS slice with scalar arithmetic */
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if ((int)blockIdx.x * W + wave >= n_workers) return; /* the last workgroup of a launch whose worker count is no multiple of W */
    const int lane = (int)__lane_id(), c_cols = (P.width + 15) >> 4, c_rows = (P.height + 15) >> 4, n_cell = c_cols * c_rows;
    __builtin_amdgcn_s_setprio(3);
    uint32_t ovf = 0;
  for (;;) {
    /* lane 0 draws; the ticket reaches the wave's other lanes through a scalar register.  The wave meets first (svt_intra_kernel: without a
     * convergent operation here the compiler threads lane 0's two `if`s into a path of its own around the loop) */
    tq_block_sync();
    int drawn = 0;
    if (lane == 0) drawn = atomicAdd(&P.sync[0], 1);
    const int ticket = __builtin_amdgcn_readfirstlane(drawn);
    if (ticket >= 3 * n_cell) break;
    const int plane = ticket % 3;
    /* the n-th cell in anti-diagonal order (encdec_core.h: the same text runs on the host, where the order is checked for every grid shape) */
    int cr, cc;
    svt_intra_cell_of_ticket(ticket / 3, c_rows, c_cols, &cr, &cc);
    const int cell = cr * c_cols + cc;
    int32_t  *done = P.sync + 2 + plane * n_cell;
    /* what the cell belongs to: the unit at the origin of its 2 x 2 cell group decides (a 32x32 block starts there or nowhere in the group), so
       the four cells of a group agree whatever the grid holds */
    const int  br = cr & ~1, bc = cc & ~1;                                      /* first cell of the group */
    const int  ub_r = br * 2, ub_c = bc * 2;                                     /* its first 8x8 unit */
    const svt_lf_mode_info b0 = P.mi[ub_r * P.mi_stride + ub_c];
    const bool big = b0.sb_type == 9 && !(b0.is_inter && P.mixed) && ub_r + 4 <= P.mi_rows && ub_c + 4 <= P.mi_cols; /* a 32x32 block coded in this pass */
    if (big && !(cr == br && cc == bc + 1)) continue;                            /* its top-right cell's ticket codes it and sets the four flags */
    const int ur0 = cr * 2, uc0 = cc * 2;
    if (lane == 0) {
        /* (r, c - 1) and (r - 1, c); for the 32x32 block at (br, bc): its lowest left neighbour (br + 1, bc - 1) and its rightmost above
           neighbour (br - 1, bc + 1) -- the flags of the cells before them on their row / column were waited for by THEIR owners */
        const int wl_r = big ? br + 1 : cr, wl_c = (big ? bc : cc) - 1;
        const int wa_r = (big ? br : cr) - 1, wa_c = big ? bc + 1 : cc;
        if (wl_c >= 0) while (__hip_atomic_load(&done[wl_r * c_cols + wl_c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) __builtin_amdgcn_s_sleep(2);
        if (wa_r >= 0) while (__hip_atomic_load(&done[wa_r * c_cols + wa_c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) __builtin_amdgcn_s_sleep(2);
    }
    tq_block_sync(); /* the wave's reference-sample loads stay behind lane 0's flag loads */
    /* the 8x8 units of the cell (of the 32x32 block: only its first unit starts a block) in z-order */
    const int nu = big ? 1 : 4, u_r = big ? ub_r : ur0, u_c = big ? ub_c : uc0;
    for (int z = 0; z < nu; z++) {
        const int r = (z >> 1) & 1, c = z & 1;
        const int ur = u_r + r, uc = u_c + c;
        if (ur >= P.mi_rows || uc >= P.mi_cols) continue;
        const svt_lf_mode_info b = P.mi[ur * P.mi_stride + uc];
        const int sub = b.sb_type == 0; /* an 8x8 unit of four 4x4 luma blocks + one 4x4 chroma block per plane */
        const int w8 = b.sb_type == 3 || sub ? 1 : b.sb_type == 6 ? 2 : b.sb_type == 9 ? 4 : 0;
        if (b.is_inter && P.mixed) continue;
        if (w8 == 0 || b.is_inter) { if (lane == 0) atomicOr(P.status, 1); continue; }
        if ((ur % w8) || (uc % w8)) continue;
        if (w8 == 4 && !big) { if (lane == 0) atomicOr(P.status, 1); continue; } /* a 32x32 block where none can start (or one that leaves the picture): malformed */
        const int mode = plane ? b.pad_[2] : b.pad_[1];
        if (ur + w8 > P.mi_rows || uc + w8 > P.mi_cols || b.tx_size != (sub ? 0 : w8 == 1 ? 1 : w8 == 2 ? 2 : 3) || (!sub && mode > 9) || b.pad_[2] > 9) {
            if (lane == 0) atomicOr(P.status, 1);
            continue;
        }
        const int sb = (ur >> 3) * P.sb_cols + (uc >> 3);
        const int x0 = plane ? uc * 4 : uc * 8, y0 = plane ? ur * 4 : ur * 8, nn = plane ? w8 * 4 : w8 * 8;
        int eob;
        if (sub && plane == 0) { /* blocks 0..3 in the reference's order, each with its own mode (nibbles of pad_[1], pad_[0]) */
            const int m4 = (int)b.pad_[1] | (int)b.pad_[0] << 8;
            eob = 0;
            for (int q4 = 0; q4 < 4; q4++) {
                const int mq = (m4 >> (4 * q4)) & 15;
                if (mq > 9) { if (lane == 0) atomicOr(P.status, 1); continue; }
                eob |= intra_rc_block<4>(P, 0, x0 + 4 * (q4 & 1), y0 + 4 * (q4 >> 1), mq, sb, s_lds, ovf, !(q4 & 1));
            }
        }
        else if (nn == 32) eob = intra_rc_block<32>(P, plane, x0, y0, mode, sb, s_lds, ovf);
        else if (nn == 16) eob = intra_rc_block<16>(P, plane, x0, y0, mode, sb, s_lds, ovf);
        else if (nn == 8) eob = intra_rc_block<8>(P, plane, x0, y0, mode, sb, s_lds, ovf);
        else eob = intra_rc_block<4>(P, plane, x0, y0, mode, sb, s_lds, ovf);
        if (eob && lane == 0) P.nz[ur * P.mi_stride + uc] = 1; /* the three planes of a block may all store the same 1 */
    }
    /* publish the cell (the four cells of a 32x32 block): its reconstruction reaches memory before the flag does */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* every (write-through) store of this wave has completed */
    tq_block_sync(); /* ... and lane 0's flag store stays behind it */
    if (lane == 0) {
        if (big) {
            _Pragma("unroll") for (int k = 0; k < 4; k++) {
                const int rr = br + (k >> 1), c2 = bc + (k & 1);
                if (rr < c_rows && c2 < c_cols) __hip_atomic_store(&done[rr * c_cols + c2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else __hip_atomic_store(&done[cell], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
    /* the tickets have run out: the worker's overflow count, one vector atomic per worker that saw any (every lane of the wave is here:
       the break above is uniform) */
    if (overflow) {
        const int s = wave_sum((int)ovf);
        if (s && lane == 0) atomicAdd(overflow, (uint32_t)s);
    }
}

} // namespace

/* internal launcher (declared in svt_ctx.h; the entry points are in encdec.hip).  Of *p: pred (may be null planes), recon, d_lf_mi, d_qcoeff,
 * d_eob_map (inputs) and d_nz; src, d_dqcoeff and d_mc_mi are not looked at.  d_status_grid: |= 1 where the grid is malformed; d_overflow
 * (may be null) is ADDED to.  Worker count and the clearing of the sync area: svt_intra_launch's rules. */
int32_t svt_intra_rc_launch(svt_hip_ctx *ctx, const svt_encdec_picture *p, int32_t width, int32_t height, int32_t mi_stride, const svt_quant_tables *d_qtabs,
                            const uint32_t iscan_off[16], int32_t *d_sync, int32_t *d_status_grid, uint32_t *d_overflow, int32_t mixed) {
    intra_pic_dev P;
    memset(&P, 0, sizeof P);
    P.pred[0] = p->pred.y; P.pred[1] = p->pred.u; P.pred[2] = p->pred.v;
    P.rec[0] = p->recon.y; P.rec[1] = p->recon.u; P.rec[2] = p->recon.v;
    P.pred_stride[0] = p->pred.y_stride; P.pred_stride[1] = p->pred.uv_stride;
    P.rec_stride[0] = p->recon.y_stride; P.rec_stride[1] = p->recon.uv_stride;
    P.mi = p->d_lf_mi; P.mi_stride = mi_stride; P.mi_rows = height >> 3; P.mi_cols = width >> 3;
    P.sb_cols = (width + 63) >> 6; P.sb_rows = (height + 63) >> 6; P.width = width; P.height = height;
    P.qtabs = d_qtabs;
    for (int i = 0; i < 16; i++) P.iscan_off[i] = iscan_off[i];
    P.qcoeff = p->d_qcoeff; P.eob_map = p->d_eob_map; P.nz = p->d_nz; P.sync = d_sync; P.status = d_status_grid; P.mixed = mixed;
    const int n_cell = ((width + 15) >> 4) * ((height + 15) >> 4); /* 16x16 luma cells: the unit of the wavefront */
    HIP_TRY(hipMemsetAsync(d_sync, 0, (size_t)(2 + 3 * n_cell) * sizeof(int32_t), ctx->stream));
    /* numbers of 64-lane WORKERS: the knobs and their order are svt_intra_launch's */
    static const int wk_per_cu = [] { const char *e = getenv("SVT_HIP_INTRA_WG_PER_CU"); return e && atoi(e) > 0 ? atoi(e) : 2; }();
    static const int wk_cap = [] { const char *e = getenv("SVT_HIP_INTRA_WGS"); return e && atoi(e) > 0 ? atoi(e) : 0; }();
    int workers = ctx->cu_count * wk_per_cu;
    const int cap = ctx->intra_wgs > 0 ? ctx->intra_wgs : wk_cap; /* the context's setting (svt_hip_ctx_set_intra_workgroups) before the environment's */
    if (cap && workers > cap) workers = cap;
    if (workers > 3 * n_cell) workers = 3 * n_cell;
    hipLaunchKernelGGL(svt_intra_rc_kernel, dim3((workers + INTRA_W - 1) / INTRA_W), dim3(64 * INTRA_W), 0, ctx->stream, P, workers, d_overflow);
    HIP_TRY(hipGetLastError());
    return SVT_HIP_OK;
}
