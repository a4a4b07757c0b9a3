/* rc_core.h -- the per-block body of the reconstruction kernels: quantised coefficients -> dequantise -> inverse DCT / ADST -> add to the
 * prediction -> clip, of ONE N x N block by N lanes of a wave: the dequantiser of a decoder in front of tq_recon_tail (tq_core.h), the
 * reconstruction half that the encode bodies run too (file comment of recon_kernel.hip).  Shared by the batch kernel (recon_kernel.hip:
 * inter pictures, prediction read from memory) and the intra decode kernel (intra_recon_kernel.hip: prediction computed in registers from
 * the neighbours' reconstruction), so that the decode pass has one copy of every rule.  Device code only; everything is internal linkage. */
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

/* One block.  k: its descriptor (recon_*, tx_type); active: false for the idle slots of a partly filled workgroup
 * (they run along with eob 0 and store nothing); i: the lane's row (first pass) / column (second pass); t: the block's LDS
 * tile; prow: row i of the prediction, packed; qrow: row i of the quantised coefficients, packed (zeros when eob is 0); dqp: the
 * table's dequant pair (DC low half, AC high half).  Returns how many of the lane's coefficients overflowed 16 bits. */
/* WT: tq_recon_tail's (intra_recon_kernel.hip) */
template <int N, bool WT = false>
__device__ __forceinline__ uint32_t rc_block_body(const svt_tq_block &k, const bool active, const int i, int32_t *t, const uint32_t (&prow)[N / 4],
                                                  const uint32_t (&qrow)[N / 2], const uint32_t dqp, const int eob, uint8_t *recon_base) {
    const int dq_dc = (int16_t)dqp, dq_ac = (int16_t)(dqp >> 16);
    int32_t   dq[N];
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
    tq_recon_tail<N, WT>(k, active, i, t, prow, dq, (N == 32) ? SVT_DCT_DCT : k.tx_type, eob, recon_base);
    return ovf;
}

} // namespace
#endif
