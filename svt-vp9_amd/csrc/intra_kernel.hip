/*
 * intra_kernel.hip -- the encode pass of an INTRA picture (gfx950): reference samples, the ten VP9 predictors, transform /
 * quantisation / reconstruction of every block, in the dependency order intra prediction imposes.
 *
 * Replaces, for a picture whose blocks are all intra (key frames and intra-refresh pictures), the per-block body of encode_pass_sb
 * (Source/Lib/Codec/EbEncDecProcess.c:3680-4160):
 *   generate_intra_reference_samples (:1128-1310; the neighbour arrays of Codec/EbNeighborArrays.c:107-240 hold the block's
 *   unfiltered reconstruction, so the reference samples are read straight from the reconstruction plane here)
 *   -> intra_prediction (Codec/EbIntraPrediction.c:16) -> eb_vp9_predict_intra_block / build_intra_predictors
 *      (VPX/vp9_reconintra.c:249-408) -> the predictors of VPX/intrapred.c:22-416
 *   -> perform_coding_loop (:365-587) with the transform type of the luma mode (eb_vp9_intra_mode_to_tx_type_lookup,
 *      vp9_reconintra.c:20-31; chroma and 32x32: DCT_DCT) -> tq_block_body (tq_core.h, the body the batch kernels use).
 * Scope: blocks of 4x4 (four to an 8x8 unit, each with its own mode), 8x8, 16x16 and 32x32 with the transform of their own size, inside
 * the picture -- what the reference codes in an intra picture whose dimensions are multiples of 8.  None of them reads the
 * above-right NEIGHBOUR BLOCK (have_right = 0 for blocks >= 8x8, EbEncDecProcess.c:1146; a 4x4 block in the left half of its unit
 * reads four above-right samples, which belong to the unit above or to the 4x4 block coded just before it) and none crosses the
 * picture edge.
 *
 * Parallelism: a block needs the reconstruction of its left, above and above-left neighbours -- and nothing else: without the
 * above-right neighbour the reference's z-order is only ONE of the orders that give its result.  The picture is cut into 32x32 luma
 * areas (the largest block here); the blocks of an area are coded one after the other (z-order) and area (r, c) can start when
 * (r, c - 1) and (r - 1, c) are done: an anti-diagonal wavefront over the areas, times three independent planes.  One 64-lane
 * WORKER (a wave) codes one (area, plane) at a time; the workers (persistent) take TICKETS (an atomic counter) that enumerate
 * the (area, plane) pairs diagonal by diagonal, so a worker only ever waits for tickets smaller than its own -- which are held by
 * workers that already run or are done: no deadlock whatever the dispatch order, no co-residency requirement.  Four workers are
 * packed into one 256-thread workgroup (see svt_intra_kernel): they share nothing but the launch.  A block is N x N
 * with N lanes active (lane i = row i of the prediction, then column / row i of the transform); the chain of dependent blocks, not
 * the lane count, bounds the speed: a 2160p key frame is 187 diagonals of at most 68 areas.  This kernel is latency-bound by design (one picture in a GOP); it shares the GPU with
 * the batches of the inter pictures running beside it.
 * Visibility between workers (other CUs, other XCDs' L2): release fence + flag store when an area is done, flag load + acquire
 * fence before the first reference-sample load; inside a worker the block's stores are drained (workgroup fence) before the
 * next block reads them.
 */
#include <hip/hip_runtime.h>
#include "tq_core.h"
#include "encdec_core.h"
#include "intra_pred.h"
#include "intra_core.h"
#include <stdlib.h>

namespace {

#ifdef INTRA_PROF
__device__ unsigned long long g_intra_fine[8];
#define IPF(k) do { if (lane == 0) { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); atomicAdd(&g_intra_fine[k], n_ - ipf_t); ipf_t = n_; } } while (0)
#else
#define IPF(k) ((void)0)
#endif
/* one N x N transform block of plane `plane` at sample (x0, y0) of that plane; the whole worker (one wave) calls it.  lds: the
 * workgroup's LDS.  The worker's slice is derived HERE, per block: carried in registers from the kernel's top across every block size's
 * body it cost well over 100 B of scratch per lane (816 B; this way the kernel holds 676 B, its one-worker predecessor held 684). */
template <int N>
__device__ __forceinline__ int intra_block(const intra_pic_dev &P, int plane, int x0, int y0, int mode, int sb, int32_t *lds, int have_right = 0) {
    const int lane = (int)__lane_id(), c = plane ? 1 : 0;
    int32_t *const tile = lds + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) * INTRA_SLICE_DW;
    uint8_t *const edge = (uint8_t *)(tile + INTRA_TILE_DW);
    const int rs = P.rec_stride[c];
    uint8_t  *rp = P.rec[plane];
    const int have_left = x0 > 0, have_top = y0 > 0;
    const bool active = lane < N;
    const int  i = lane % N;
#ifdef INTRA_PROF
    unsigned long long ipf_t = __builtin_amdgcn_s_memtime();
#endif
    uint32_t   srow[N / 4], prow[N / 4];
    constexpr uintptr_t AM = N >= 16 ? 15 : N - 1;
    {   /* the source row does not depend on the neighbours: its load is issued first and completes under the reference-sample loads */
        const uint8_t *sp = P.src[plane] + (size_t)(y0 + i) * P.src_stride[c] + x0;
        _Pragma("unroll") for (int q = 0; q < N / 4; q++) srow[q] = 0u;
        if (active) row_load<N>(sp, ((uintptr_t)sp & AM) == 0, srow);
    }
    /* reference samples -> LDS (generate_intra_reference_samples, the paths of a block inside the picture) */
#include "intra_refs.inc"
    tq_block_sync(); /* edge[] is written and read by this wave alone */
    IPF(0); /* source issue + reference samples into LDS */
    intra_pred_row<N>(edge, mode, i, have_left, have_top, prow);
    {
        if (active && P.pred[plane]) {
            uint8_t *pp = P.pred[plane] + (size_t)(y0 + i) * P.pred_stride[c] + x0;
            row_store<N>(pp, ((uintptr_t)pp & AM) == 0, prow);
        }
    }
    IPF(1); /* prediction (+ its store) */
    svt_tq_block k;
    k.src_off = k.pred_off = 0;
    k.recon_off = (uint32_t)y0 * (uint32_t)rs + (uint32_t)x0;
    k.coeff_off = (uint32_t)sb * SVT_SB_COEFFS + (plane == 0 ? 0u : plane == 1 ? 4096u : 5120u) + svt_zorder4((x0 & (plane ? 31 : 63)) >> 2, (y0 & (plane ? 31 : 63)) >> 2) * 16u;
    k.tx_size = (uint8_t)txcfg<N>::size;
    k.tx_type = (uint8_t)((plane == 0 && N < 32) ? intra_tx_type(mode) : 0);
    k.iscan_off = P.iscan_off[k.tx_size * 4 + k.tx_type];
    k.src_stride = k.pred_stride = 0; k.recon_stride = (uint16_t)rs;
    k.qtab = (uint8_t)c; k.do_recon = 1; k.partial32 = 0; k.pad_[0] = 0;
    const int pw4 = (plane ? P.width >> 1 : P.width) >> 2, w4 = P.width >> 2, h4 = P.height >> 2;
    const int eo = plane == 0 ? 0 : w4 * h4 + (plane == 2 ? (w4 >> 1) * (h4 >> 1) : 0);
    int32_t *t = tile + (lane / N) * (N * (N + 1)); /* the idle slots of the wave run along on tiles of their own */
    const int eob = tq_block_body<N, false, false, INTRA_WT>(k, active, i, t, srow, prow, P.qtabs, P.iscan, P.qcoeff, P.dqcoeff,
                                                   P.eob_map + eo + (y0 >> 2) * pw4 + (x0 >> 2), nullptr, nullptr, nullptr, nullptr, nullptr, rp);
    IPF(2); /* transform / quantisation / reconstruction */
    /* the block's reconstruction is read by the next block of this wave: drain the stores */
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    tq_block_sync();
    IPF(3); /* store drain */
    return __builtin_amdgcn_readfirstlane(eob);
}

#ifndef INTRA_WAVES_PER_EU
#define INTRA_WAVES_PER_EU 4
#endif
/* Register budget: left alone the compiler takes 308 VGPRs for this kernel -- one such wave per CU, resident for milliseconds, leaves
 * its SIMD room for two motion-estimation waves instead of five, i.e. the CU two ME workgroups instead of five (measured in the step:
 * + 4 ms per key frame, whatever the number of workers of this launch).  Held to 128 it spills the 32x32 path's transform rows
 * to scratch, but displaces one ME wave, not three.
 *
 * Packing: a workgroup is W independent 64-lane WORKERS (waves), each with its own slice of the LDS.  Beside the 2160p ME instance
 * (five four-wave workgroups fill a CU: 96 VGPRs x 5 waves per SIMD, 25 of 128 LDS granules each) a 128-VGPR wave takes the registers
 * of one ME wave on its SIMD, i.e. one whole ME workgroup off its CU -- as a one-wave workgroup just as much as four waves, one per
 * SIMD, do.  W = 4 puts four workers into that one hole: 4 x (8 448 + 128) B = 34 304 B = 27 LDS granules of 1 280 B, which with four ME
 * workgroups is 127 of 128.
 * The workers of a workgroup NEVER meet: they draw different tickets, loop different numbers of times and leave at different
 * moments, so there is no workgroup barrier anywhere in this kernel (one s_barrier would hang it) -- every rendezvous is of the lanes
 * of ONE wave (tq_block_sync: LDS and memory accesses of a wave are issued in order; what has to be kept is the compiler's order).
 * Deadlock: a worker waits only at the flags of cells with SMALLER tickets than its own.  A ticket exists only because a worker that
 * was already running drew it, and a running wave keeps running whatever its workgroup-mates do (no barrier, no shared state): so
 * the holder of the smallest unfinished ticket waits for nothing and finishes, then the next -- whatever the dispatch order, however
 * few workers are resident, and whichever of them share a workgroup. */
#ifdef INTRA_NUM_VGPR
__attribute__((amdgpu_num_vgpr(INTRA_NUM_VGPR)))
#endif
__global__ __launch_bounds__(64 * INTRA_W) __attribute__((amdgpu_waves_per_eu(INTRA_WAVES_PER_EU, INTRA_WAVES_PER_EU))) void svt_intra_kernel(const intra_pic_dev P, const int n_workers) {
    /* the walk (its comments give the ticket draw, the 32x32 rule, the wait targets and the drain): one text for this kernel and
       svt_intra_rc_kernel; this kernel opts into the walk's -DINTRA_PROF timers */
#ifdef INTRA_PROF
#define INTRA_WALK_PROF
#endif
#define INTRA_WALK_BLOCK(N, plane, x0, y0, mode, sb, have_right) intra_block<N>(P, plane, x0, y0, mode, sb, s_lds, have_right)
#include "intra_walk.inc"
#undef INTRA_WALK_BLOCK
}

/* stand-in decision for an intra picture (no claim of coding efficiency; the public API's callback replaces it): 16x16 blocks with
 * DC prediction, 8x8 where a 16x16 block would cross the picture edge */
__global__ __launch_bounds__(256) void svt_md_intra_default_kernel(svt_lf_mode_info *mi, int mi_stride, int mi_rows, int mi_cols, int filter_level) {
    const int u = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (u >= mi_rows * mi_cols) return;
    const int r = u / mi_cols, c = u % mi_cols;
    const int fit16 = (r & ~1) + 2 <= mi_rows && (c & ~1) + 2 <= mi_cols;
    svt_lf_mode_info m;
    m.sb_type = fit16 ? 6 : 3; m.tx_size = fit16 ? 2 : 1; m.skip = 0; m.is_inter = 0; m.filter_level = (uint8_t)filter_level;
    m.pad_[0] = m.pad_[1] = m.pad_[2] = 0;
    mi[r * mi_stride + c] = m;
}

} // namespace

/* internal launchers (declared in svt_ctx.h; the entry points are in encdec.hip) */
int32_t svt_intra_launch(svt_hip_ctx *ctx, const svt_encdec_picture *p, int32_t width, int32_t height, int32_t mi_stride, const svt_quant_tables *d_qtabs,
                         const int16_t *d_iscan, const uint32_t iscan_off[16], int32_t *d_sync, int32_t *d_status, int32_t mixed) {
    intra_pic_dev P;
    int           workers = 0;
    if (const int32_t e = intra_launch_prepare(ctx, p, width, height, mi_stride, d_qtabs, iscan_off, d_sync, d_status, mixed, true, d_iscan, P, &workers)) return e;
    hipLaunchKernelGGL(svt_intra_kernel, dim3((workers + INTRA_W - 1) / INTRA_W), dim3(64 * INTRA_W), 0, ctx->stream, P, workers);
    HIP_TRY(hipGetLastError());
    return SVT_HIP_OK;
}

int32_t svt_md_intra_default_launch(svt_hip_ctx *ctx, svt_lf_mode_info *d_lf_mi, int32_t mi_stride, int32_t mi_rows, int32_t mi_cols, int32_t filter_level) {
    hipLaunchKernelGGL(svt_md_intra_default_kernel, dim3((mi_rows * mi_cols + 255) / 256), dim3(256), 0, ctx->stream, d_lf_mi, mi_stride, mi_rows, mi_cols, filter_level);
    HIP_TRY(hipGetLastError());
    return SVT_HIP_OK;
}
