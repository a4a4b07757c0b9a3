/* intra_core.h -- what the two wavefront kernels of an intra picture share: the picture record their launchers fill, the access forms that
 * make a block's reconstruction visible to the workers that predict from it, the layout of a worker's LDS slice, and the host preamble of
 * their launchers (intra_launch_prepare).  Used by intra_kernel.hip (the encode pass: source -> coefficients + reconstruction) and
 * intra_recon_kernel.hip (the decode pass: coefficients -> reconstruction).  The wavefront walk itself and the reference-sample staging
 * are shared as TEXT: intra_walk.inc, included inside both kernels' bodies, and intra_refs.inc, inside both block bodies -- there is one
 * walk, not two that agree.  Everything here is internal linkage. */
#ifndef SVT_INTRA_CORE_H
#define SVT_INTRA_CORE_H
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "svt_ctx.h"

namespace {

struct intra_pic_dev {
    const uint8_t *src[3];
    uint8_t       *pred[3];  /* may be null: the prediction is then not stored */
    uint8_t       *rec[3];
    int32_t        src_stride[2], pred_stride[2], rec_stride[2];
    const svt_lf_mode_info *mi;
    int32_t        mi_stride, mi_rows, mi_cols, sb_cols, sb_rows, width, height;
    const svt_quant_tables *qtabs;
    const int16_t *iscan;
    uint32_t       iscan_off[16];
    int16_t       *qcoeff, *dqcoeff;
    uint16_t      *eob_map;
    uint8_t       *nz;
    int32_t       *sync;    /* [0] ticket counter, [2 + plane * n_cell + cell] done flags (16x16 luma cells); zeroed before the launch */
    int32_t       *status;  /* |= 1: a malformed grid was seen */
    int32_t        mixed;   /* 1: an inter picture with some intra blocks: inter blocks are skipped (the batch coded them) */
};

/* Visibility of a block's reconstruction to the workers that predict from it (other CUs, other XCDs): written through and read
 * with agent-scope accesses (the deblocking kernel's seam-row scheme), NOT with a release / acquire fence pair per area: such a pair
 * is buffer_wbl2 sc1 + buffer_inv sc1 -- write-back and invalidation of the XCD's whole L2 -- 18 000 times per 2160p key frame, paid by
 * every kernel that runs beside this one (measured in the step: a key frame cost + 4 ms of step time with the fences, however few
 * workers coded it).  -DINTRA_FENCES restores the fence form (3-12 % faster when the pass has the GPU to itself). */
#ifdef INTRA_FENCES
#define INTRA_WT false
#define INTRA_LD(p) (*(p))
#else
#define INTRA_WT true
#define INTRA_LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif
/* a worker's slice of the workgroup's LDS: the transform tiles (two 32 x 33 dword tiles: the idle half of the wave runs along on its
 * own), then the 128 reference samples */
#define INTRA_TILE_DW  (2 * 32 * 33)
#define INTRA_SLICE_DW (INTRA_TILE_DW + 128 / 4)
#define INTRA_W        4 /* workers per workgroup */

/* Host: what both launchers do in front of their hipLaunchKernelGGL.  Fills P from the picture (encode: also the source planes, the
 * inverse scans and dqcoeff; the decode pass leaves them null), clears the sync area on the stream and returns the number of 64-lane
 * WORKERS in *workers (the names of the knobs date from one worker per workgroup); the launch is ceil(workers / INTRA_W) workgroups of
 * 64 * INTRA_W threads. */
inline int32_t intra_launch_prepare(svt_hip_ctx *ctx, const svt_encdec_picture *p, int32_t width, int32_t height, int32_t mi_stride, const svt_quant_tables *d_qtabs,
                                    const uint32_t iscan_off[16], int32_t *d_sync, int32_t *d_status, int32_t mixed, bool encode, const int16_t *d_iscan,
                                    intra_pic_dev &P, int *workers_out) {
    memset(&P, 0, sizeof P);
    if (encode) {
        P.src[0] = p->src.y; P.src[1] = p->src.u; P.src[2] = p->src.v;
        P.src_stride[0] = p->src.y_stride; P.src_stride[1] = p->src.uv_stride;
        P.iscan = d_iscan; P.dqcoeff = p->d_dqcoeff;
    }
    P.pred[0] = p->pred.y; P.pred[1] = p->pred.u; P.pred[2] = p->pred.v;
    P.rec[0] = p->recon.y; P.rec[1] = p->recon.u; P.rec[2] = p->recon.v;
    P.pred_stride[0] = p->pred.y_stride; P.pred_stride[1] = p->pred.uv_stride;
    P.rec_stride[0] = p->recon.y_stride; P.rec_stride[1] = p->recon.uv_stride;
    P.mi = p->d_lf_mi; P.mi_stride = mi_stride; P.mi_rows = height >> 3; P.mi_cols = width >> 3;
    P.sb_cols = (width + 63) >> 6; P.sb_rows = (height + 63) >> 6; P.width = width; P.height = height;
    P.qtabs = d_qtabs;
    for (int i = 0; i < 16; i++) P.iscan_off[i] = iscan_off[i];
    P.qcoeff = p->d_qcoeff; P.eob_map = p->d_eob_map; P.nz = p->d_nz; P.sync = d_sync; P.status = d_status; P.mixed = mixed;
    const int n_cell = ((width + 15) >> 4) * ((height + 15) >> 4); /* 16x16 luma cells: the unit of the wavefront */
    HIP_TRY(hipMemsetAsync(d_sync, 0, (size_t)(2 + 3 * n_cell) * sizeof(int32_t), ctx->stream));
    /* (function-local statics with an initialiser: initialised once, thread-safely -- several contexts may launch from several threads) */
    static const int wk_per_cu = [] { const char *e = getenv("SVT_HIP_INTRA_WG_PER_CU"); return e && atoi(e) > 0 ? atoi(e) : 2; }(); /* two: a diagonal's tickets are then mostly held by workers already waiting at their flags (2160p, 16x16 DC: 4.77 -> 4.34 ms) */
    static const int wk_cap = [] { const char *e = getenv("SVT_HIP_INTRA_WGS"); return e && atoi(e) > 0 ? atoi(e) : 0; }(); /* deployment knob: fewer workers = a longer pass that leaves more of the device to what runs beside it (bench.py: 128) */
    int workers = ctx->cu_count * wk_per_cu;
    const int cap = ctx->intra_wgs > 0 ? ctx->intra_wgs : wk_cap; /* the context's setting (svt_hip_ctx_set_intra_workgroups) before the environment's */
    if (cap && workers > cap) workers = cap;
    if (workers > 3 * n_cell) workers = 3 * n_cell;
    *workers_out = workers;
    return SVT_HIP_OK;
}

} // namespace
#endif
