/*
 * intra_recon_kernel.hip -- the DECODE pass of an intra picture's blocks (gfx950): reference samples, the ten VP9 predictors, then
 * dequantisation / inverse transform / reconstruction of every block from its quantised coefficients and eob, in the dependency order
 * intra prediction imposes.  The coefficient-driven twin of svt_intra_kernel (intra_kernel.hip): what that kernel does with the
 * source in hand (tq_block_body: forward transform, quantiser, inverse) this one does from what a frame reader returned
 * (rc_block_body, rc_core.h: the body svt_rc_kernel runs for inter pictures) -- the reconstruction process of the VP9 specification for
 * intra blocks, i.e. the prediction of VPX/vp9_reconintra.c:249-408 followed by eb_vp9_idct*_add / eb_vp9_iht*_add (VPX/vp9_idct.c:111-189).
 *
 * THE WALK IS svt_intra_kernel's: the same text, intra_walk.inc, included by both kernels (its comments and intra_kernel.hip's give the
 * rules and their reasons), and the reference samples are intra_refs.inc in both block bodies.  The walk looks at the mode-info grid alone,
 * never at coefficients or eobs, so a picture terminates whatever the coefficient arrays hold.
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
    /* reference samples -> LDS (generate_intra_reference_samples, the paths of a block inside the picture) */
#include "intra_refs.inc"
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
    uint32_t ovf = 0;
    /* the walk: one text for svt_intra_kernel and this kernel (INTRA_WALK_PROF is not defined: -DINTRA_PROF changes nothing here) */
#define INTRA_WALK_BLOCK(N, plane, x0, y0, mode, sb, have_right) intra_rc_block<N>(P, plane, x0, y0, mode, sb, s_lds, ovf, have_right)
#include "intra_walk.inc"
#undef INTRA_WALK_BLOCK
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
 * (may be null) is ADDED to.  Worker count and the clearing of the sync area: intra_launch_prepare (intra_core.h), as for svt_intra_launch. */
int32_t svt_intra_rc_launch(svt_hip_ctx *ctx, const svt_encdec_picture *p, int32_t width, int32_t height, int32_t mi_stride, const svt_quant_tables *d_qtabs,
                            const uint32_t iscan_off[16], int32_t *d_sync, int32_t *d_status_grid, uint32_t *d_overflow, int32_t mixed) {
    intra_pic_dev P;
    int           workers = 0;
    if (const int32_t e = intra_launch_prepare(ctx, p, width, height, mi_stride, d_qtabs, iscan_off, d_sync, d_status_grid, mixed, false, nullptr, P, &workers)) return e;
    hipLaunchKernelGGL(svt_intra_rc_kernel, dim3((workers + INTRA_W - 1) / INTRA_W), dim3(64 * INTRA_W), 0, ctx->stream, P, workers, d_overflow);
    HIP_TRY(hipGetLastError());
    return SVT_HIP_OK;
}
