/* rc_core.h -- the per-block body of the reconstruction kernels: quantised coefficients -> dequantise -> inverse DCT / ADST -> add to the
 * prediction -> clip, of ONE N x N block by N lanes of a wave (the second half of tq_block_body, tq_core.h, on its own; file comment of
 * recon_kernel.hip).  Shared by the batch kernel (recon_kernel.hip: inter pictures, prediction read from memory) and the intra decode
 * kernel (intra_recon_kernel.hip: prediction computed in registers from the neighbours' reconstruction), so that the decode pass has one
 * copy of every rule.  Device code only; everything is internal linkage. */
#ifndef SVT_RC_CORE_H
#define SVT_RC_CORE_H
#include <hip/hip_runtime.h>
#include "tq_core.h"

namespace {

/* the picture's eob map entry of the block at position code p (encdec.hip: svt_tq_skip_kernel writes the same place) */
__device__ __forceinline__ int rc_eob_of_pos(uint32_t p, const svt_tq_pic_geom *g, const uint16_t *eob_map) {
    const int plane = (int)(p >> 22) & 3, y4 = (int)(p >> 11) & 0x7ff, x4 = (int)p & 0x7ff;
    const int w4 = g->width >> 2, h4 = g->height >> 2;
    const int pw4 = plane ? w4 >> 1 : w4;
    const int off = plane == 0 ? 0 : w4 * h4 + (plane == 2 ? (w4 >> 1) * (h4 >> 1) : 0);
    return eob_map[off + y4 * pw4 + x4];
}

/* One block.  k: its descriptor (pred_*, recon_*, coeff_off, tx_type, qtab); active: false for the idle slots of a partly filled
 * workgroup (they run along with eob 0 and store nothing); i: the lane's row (first pass) / column (second pass); t: the block's LDS
 * tile; prow: row i of the prediction, packed; qrow: row i of the quantised coefficients, packed (zeros when eob is 0); dqp: the
 * table's dequant pair (DC low half, AC high half).  Returns how many of the lane's coefficients overflowed 16 bits. */
/* WT: the reconstruction is stored write-through (agent-scope dword stores, tq_block_body's form), for a caller whose neighbour blocks
 * are read by other workgroups of the SAME launch (intra_recon_kernel.hip) */
template <int N, bool WT = false>
__device__ __forceinline__ uint32_t rc_block_body(const svt_tq_block &k, const bool active, const int i, int32_t *t, const uint32_t (&prow)[N / 4],
                                                  const uint32_t (&qrow)[N / 2], const uint32_t dqp, const int eob, uint8_t *recon_base) {
    constexpr int LS = N + 1;            /* padded LDS row stride in dwords */
    const int  tx_type = (N == 32) ? SVT_DCT_DCT : k.tx_type;
    const bool col_adst = tx_type == SVT_ADST_DCT || tx_type == SVT_ADST_ADST;
    const bool row_adst = tx_type == SVT_DCT_ADST || tx_type == SVT_ADST_ADST;
    const int  dq_dc = (int16_t)dqp, dq_ac = (int16_t)(dqp >> 16);
    int32_t  v[N], o[N], dq[N];
    uint32_t ovf = 0;
    /* ---- dequantise row i (= vertical frequency i) ---- */
    _Pragma("unroll") for (int kk = 0; kk < N; kk++) {
        const int qv = (int16_t)(qrow[kk >> 1] >> (16 * (kk & 1)));
        int       p = qv * ((i | kk) != 0 ? dq_ac : dq_dc);
        if constexpr (N == 32) p /= 2;
        const int dv = (int16_t)p;
        ovf += dv != p;
        dq[kk] = dv;
    }
    /* ---- reconstruction: recon = pred + inverse transform (rows first, then columns) ---- */
    int32_t res[N];
    _Pragma("unroll") for (int r = 0; r < N; r++) res[r] = 0;
    const bool dct_path = tx_type == SVT_DCT_DCT;
    bool dc_only = false;
    int  nrows = N;
    if (dct_path) {
        if (N == 4) dc_only = eob <= 1;
        else dc_only = eob == 1;
        if (N == 8) nrows = eob <= 12 ? 4 : 8;
        if (N == 16) nrows = eob <= 10 ? 4 : eob <= 38 ? 8 : 16;
        if (N == 32) nrows = eob <= 34 ? 8 : eob <= 135 ? 16 : 32;
    }
    if (eob != 0 && !dc_only) {
        if (i < nrows) inv1d<N>(dq, o, row_adst);
        else { _Pragma("unroll") for (int kk = 0; kk < N; kk++) o[kk] = 0; }
        _Pragma("unroll") for (int kk = 0; kk < N; kk++) t[i * LS + kk] = (int16_t)o[kk];
    } else if (eob != 0 && i == 0) {
        t[0] = dq[0];
    }
    tq_block_sync();
    if (eob != 0 && !dc_only) {
        _Pragma("unroll") for (int r = 0; r < N; r++) v[r] = t[r * LS + i];
        inv1d<N>(v, o, col_adst);
        _Pragma("unroll") for (int r = 0; r < N; r++) res[r] = ((int16_t)o[r] + (1 << (txcfg<N>::shift - 1))) >> txcfg<N>::shift;
    } else if (eob != 0) {
        /* eb_vp9_idct*_1_add_c: inv_txfm.c:174, 368, 784, 1241 */
        int32_t d = tx_rsw((int16_t)t[0] * TX_C16);
        d = tx_rsw(d * TX_C16);
        const int32_t a1 = (d + (1 << (txcfg<N>::shift - 1))) >> txcfg<N>::shift;
        _Pragma("unroll") for (int r = 0; r < N; r++) res[r] = a1;
    }
    tq_block_sync(); /* (the DC lane's t[0] has been read) */
    /* residual column i -> LDS -> row i; reconstruction = clip(pred row + residual row), stored as dwords */
    _Pragma("unroll") for (int r = 0; r < N; r++) t[r * LS + i] = res[r];
    tq_block_sync();
    if (active && recon_base) { /* (null: the block named a reconstruction set the caller did not pass) */
        uint8_t *d = recon_base + k.recon_off + (size_t)i * k.recon_stride;
        uint32_t rw[N / 4];
        _Pragma("unroll") for (int q = 0; q < N / 4; q++) {
            uint32_t w = 0;
            _Pragma("unroll") for (int b = 0; b < 4; b++)
                w |= (uint32_t)clip_add((int)((prow[q] >> (8 * b)) & 0xff), t[i * LS + 4 * q + b]) << (8 * b);
            rw[q] = w;
        }
        if constexpr (WT) {
            _Pragma("unroll") for (int q = 0; q < N / 4; q++) __hip_atomic_store((uint32_t *)d + q, rw[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else row_store<N>(d, ((uintptr_t)d & (N >= 16 ? 15 : N - 1)) == 0, rw);
    }
    return ovf;
}

} // namespace
#endif
