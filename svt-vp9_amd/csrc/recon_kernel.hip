/*
 * recon_kernel.hip -- quantised coefficients -> dequantise -> inverse DCT / ADST -> add to the prediction -> clip, for batches of VP9
 * transform blocks (gfx950): the arithmetic of a decoder's reconstruction, run by the reconstruction half of the encode pass (tq_core.h).
 *
 * What a non-high-bit-depth decoder does per transform block (the VP9 specification's reconstruction process; the same arithmetic as the
 * tail of perform_coding_loop, Source/Lib/Codec/EbEncDecProcess.c:365-587: eb_vp9_quantize_b[_32x32]'s dqcoeff, VPX/quantize.c:112-254, then
 * eb_vp9_idct*_add / eb_vp9_iht*_add, VPX/vp9_idct.c:111-189, VPX/inv_txfm.c):
 *     dqcoeff = (int16)(qcoeff * dequant[0 for DC, 1 for AC]), 32x32: (int16)(qcoeff * dequant / 2), the division towards zero;
 *     rows first, then columns, with the eob shortcuts of vp9_idct.c (DC only; 4 / 8 / 16 rows of the larger transforms);
 *     recon = clip(pred + ((column result + half) >> shift)); a block with eob 0 copies the prediction.
 * A dequantised product that does not fit in 16 signed bits makes a stream non-conformant; the wrapped value is used (as the encode pass
 * does) and the coefficients it happened to are counted per launch (of the blocks with eob != 0: the others are not read).
 *
 * Mapping (tq_core.h's): N lanes of one wave per N x N block, 256 / N blocks per 256-thread workgroup; lane i owns ROW i of the
 * coefficients (16-byte vector loads: coeff_off is a multiple of 8 coefficients and the array 16-byte aligned) and of the prediction
 * (row_load), the row <-> column change goes through the block's N x (N + 1) dword LDS tile, ordered with tq_block_sync -- the lanes of
 * a block sit in one wave, there is no workgroup barrier.  Workgroups are persistent and walk their XCD's eighth of the list (tq_walk_of).
 * The inverse and the clip-add are the encode pass's own code: rc_block_body (rc_core.h, shared with the intra decode kernel,
 * intra_recon_kernel.hip) dequantises and calls tq_recon_tail (tq_core.h), which tq_block_body calls behind its quantiser
 * (tests/test_gpu_decode.py compares the two passes' reconstruction bytes, tests/test_gpu_recon_edges.py holds the tail to the reference's
 * recorded bytes on coefficients the forward path never makes).  No inline assembly; every store is a vector store.
 *
 * Two launch forms: descriptor lists (svt_hip_recon_batch_device: svt_hip_tq_batch_device's svt_tq_block lists, eob per list entry) and
 * the encode pass's device-built position codes (svt_rc_launch_device_lists, used by svt_hip_decode_batch_device: a block's eob is read
 * from its picture's eob map at the block's origin unit and also left in list order for svt_tq_skip_kernel).
 */
#include <hip/hip_runtime.h>
#include "tq_core.h"
#include "rc_core.h"
#include "wave_ops.h"

namespace {

/* eob_in: the blocks' eobs in list order (descriptor lists).  dc.pos != null: position codes; the eob comes from the picture's eob map
 * (eob_maps + picture * dc.geom_stride holds the pointer to it) and is left in eob_list in list order. */
template <int N>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(N == 32 ? 4 : 1))) void svt_rc_kernel(const uint8_t *__restrict__ pred, uint8_t *__restrict__ recon,
                                                     const svt_tq_block *__restrict__ blocks, int n_blocks, const svt_quant_tables *__restrict__ qtabs,
                                                     const int16_t *__restrict__ qcoeff, const uint16_t *__restrict__ eob_in, uint16_t *__restrict__ eob_list,
                                                     uint32_t *__restrict__ overflow, const uint8_t *const *__restrict__ recon_set, tq_dev_count dc,
                                                     const uint8_t *__restrict__ eob_maps) {
    eob_list += dc.first_block(n_blocks); /* device-built list: where this size's blocks start and how many there are */
    constexpr int BPW = 256 / N;          /* blocks per workgroup */
    constexpr int LS  = N + 1;            /* padded LDS row stride in dwords */
    __shared__ int32_t tile[BPW][N * LS];
    const int lb = threadIdx.x / N;       /* block slot inside the workgroup */
    const int i  = threadIdx.x % N;       /* row (pass 1) / column (pass 2) owned by this lane */
    const tq_walk wk = tq_walk_of((n_blocks + BPW - 1) / BPW);
    uint32_t ovf = 0;
    for (int gj = wk.first; gj < wk.per_xcd; gj += wk.step) {
        const int grp = wk.base + gj;
        if (grp * BPW >= n_blocks) break;     /* uniform: depends on the workgroup only */
        const int  blk = grp * BPW + lb;
        const bool active = blk < n_blocks;
        svt_tq_block k;
        int          eob = 0;
        if (dc.pos) { /* (uniform) the list holds position codes: the descriptor is rebuilt in registers */
            const uint32_t pc = dc.pos[active ? blk : 0];
            const svt_tq_pic_geom *g = tq_block_of_pos<N>(dc, pc, &k);
            if (active) {
                eob = rc_eob_of_pos(pc, g, *(const uint16_t *const *)(eob_maps + (size_t)svt_tq_pos_pic(pc) * dc.geom_stride));
                if (i == 0) eob_list[blk] = (uint16_t)eob;
            }
        } else {
            k = blocks[active ? blk : 0];
            if (active) eob = eob_in[blk];
        }
        uint32_t prow[N / 4], qrow[N / 2];
        _Pragma("unroll") for (int q = 0; q < N / 4; q++) prow[q] = 0u;
        _Pragma("unroll") for (int q = 0; q < N / 2; q++) qrow[q] = 0u;
        if (active) {
            const uint8_t *pp = pred + k.pred_off + (size_t)i * k.pred_stride;
            row_load<N>(pp, ((uintptr_t)pp & (N >= 16 ? 15 : N - 1)) == 0, prow);
            if (eob) { /* row i of the coefficients: 2 N bytes per lane, consecutive lanes consecutive rows */
                const int16_t *qp = qcoeff + k.coeff_off + i * N;
                if constexpr (N == 4) { const uint2 w = *(const uint2 *)qp; qrow[0] = w.x; qrow[1] = w.y; }
                else {
                    _Pragma("unroll") for (int j = 0; j < N / 8; j++) {
                        const uint4 w = ((const uint4 *)qp)[j];
                        qrow[4 * j] = w.x; qrow[4 * j + 1] = w.y; qrow[4 * j + 2] = w.z; qrow[4 * j + 3] = w.w;
                    }
                }
            }
        }
        const uint32_t dqp = ((const uint32_t *)(qtabs + k.qtab))[4]; /* dequant[0], dequant[1]: the fifth dword of the 20-byte table */
        ovf += rc_block_body<N>(k, active, i, tile[lb], prow, qrow, dqp, eob, recon_set ? (uint8_t *)recon_set[(k.pad_[0] >> 4) & 7] : recon);
        tq_block_sync(); /* the block's tile is rewritten by its lanes' next block */
    }
    if (overflow) { /* one atomic per wave that saw any */
        const int s = wave_sum((int)ovf);
        if (s && (threadIdx.x & 63) == 0) atomicAdd(overflow, (uint32_t)s);
    }
}

/* persistent grid: a multiple of 8 workgroups (one walk per XCD, tq_walk_of), at most six per CU (nothing is known about what runs
 * beside the launch; unmeasured) */
int rc_grid(svt_hip_ctx *ctx, int ngroups) {
    const int per_xcd = (ngroups + 7) / 8, cap = (ctx->cu_count * 12 + 15) / 16;
    return 8 * (per_xcd < cap ? per_xcd : cap);
}

template <int N>
hipError_t launch_rc(svt_hip_ctx *ctx, const uint8_t *pred, uint8_t *recon, const svt_tq_block *blocks, int n, const svt_quant_tables *q, const int16_t *qc,
                     const uint16_t *eob_in, uint16_t *eob_list, uint32_t *overflow, const uint8_t *const *recon_set, tq_dev_count dc, const uint8_t *eob_maps) {
    if (n <= 0) return hipSuccess;
    constexpr int BPW = 256 / N;
    hipLaunchKernelGGL((svt_rc_kernel<N>), dim3(rc_grid(ctx, (n + BPW - 1) / BPW)), dim3(256), 0, ctx->stream, pred, recon, blocks, n, q, qc, eob_in, eob_list, overflow,
                       recon_set, dc, eob_maps);
    return hipGetLastError();
}

} // namespace

/* Reconstruction over block lists that were built ON THE DEVICE (csrc/encdec.hip), the counterpart of svt_tq_launch_device_lists: d_pos
 * holds the position codes, d_off_cnt where each size starts and how many there are, cap[s] an upper bound that only sizes the grids.
 * d_geom / d_eob_maps: the first picture's svt_tq_pic_geom / pointer to its eob map, both inside records geom_stride bytes apart.
 * d_eob_list receives the eobs in list order.  d_overflow (may be null) is ADDED to.  Internal to the library (declared in svt_ctx.h). */
int32_t svt_rc_launch_device_lists(svt_hip_ctx *ctx, const uint8_t *d_pred, uint8_t *const *recon_set, int n_set, const int32_t cap[4], const int32_t *d_off_cnt,
                                   const svt_quant_tables *d_qtabs, const int16_t *d_qcoeff, uint16_t *d_eob_list, const uint32_t *d_pos, const void *d_geom,
                                   const void *d_eob_maps, int geom_stride, const uint32_t *d_iscan_off, int sb_cols, uint32_t *d_overflow) {
    HIP_TRY(hipSetDevice(ctx->device));
    const uint8_t *const *d_set = nullptr;
    if (const int32_t e = tq_stage_recon_set(ctx, recon_set, n_set, &d_set)) return e;
    hipError_t rc = hipSuccess;
#define RC_DEV(N, S) launch_rc<N>(ctx, d_pred, nullptr, nullptr, cap[S], d_qtabs, d_qcoeff, nullptr, d_eob_list, d_overflow, d_set, \
                                  tq_dev_count{d_off_cnt, S, d_pos, (const uint8_t *)d_geom, geom_stride, d_iscan_off, sb_cols}, (const uint8_t *)d_eob_maps)
    rc = RC_DEV(4, 0);
    if (rc == hipSuccess) rc = RC_DEV(8, 1);
    if (rc == hipSuccess) rc = RC_DEV(16, 2);
    if (rc == hipSuccess) rc = RC_DEV(32, 3);
#undef RC_DEV
    HIP_TRY(rc);
    return SVT_HIP_OK;
}

/* svt_hip_tq_batch_device's lists, read the other way: d_qcoeff and d_eob are inputs, d_recon the output (include/svtvp9_hip.h) */
extern "C" int32_t svt_hip_recon_batch_device(svt_hip_ctx *ctx, const uint8_t *d_pred, uint8_t *d_recon, const svt_tq_block *d_blocks, const int32_t size_count[4],
                                              const svt_quant_tables *d_qtabs, const int16_t *d_qcoeff, const uint16_t *d_eob, uint32_t *d_overflow) {
    if (!ctx || !d_pred || !d_recon || !d_blocks || !size_count || !d_qtabs || !d_qcoeff || !d_eob) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "recon: null argument");
    if ((uintptr_t)d_qcoeff & 15) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "recon: the coefficient array must be 16-byte aligned");
    for (int s = 0; s < 4; s++)
        if (size_count[s] < 0) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "recon: negative block count");
    HIP_TRY(hipSetDevice(ctx->device));
    svt_ctx_timer timer(ctx);
    HIP_TRY(timer.begin());
    if (d_overflow) HIP_TRY(hipMemsetAsync(d_overflow, 0, sizeof(uint32_t), ctx->stream));
    const tq_dev_count none = {nullptr, 0, nullptr, nullptr, 0, nullptr, 0};
    int        off = 0;
    hipError_t rc = launch_rc<4>(ctx, d_pred, d_recon, d_blocks + off, size_count[0], d_qtabs, d_qcoeff, d_eob + off, nullptr, d_overflow, nullptr, none, nullptr);
    off += size_count[0];
    if (rc == hipSuccess) rc = launch_rc<8>(ctx, d_pred, d_recon, d_blocks + off, size_count[1], d_qtabs, d_qcoeff, d_eob + off, nullptr, d_overflow, nullptr, none, nullptr);
    off += size_count[1];
    if (rc == hipSuccess) rc = launch_rc<16>(ctx, d_pred, d_recon, d_blocks + off, size_count[2], d_qtabs, d_qcoeff, d_eob + off, nullptr, d_overflow, nullptr, none, nullptr);
    off += size_count[2];
    if (rc == hipSuccess) rc = launch_rc<32>(ctx, d_pred, d_recon, d_blocks + off, size_count[3], d_qtabs, d_qcoeff, d_eob + off, nullptr, d_overflow, nullptr, none, nullptr);
    HIP_TRY(rc);
    HIP_TRY(timer.end());
    return SVT_HIP_OK;
}
