/* intra_core.h -- what the two wavefront kernels of an intra picture share: the picture record their launchers fill, the access forms that
 * make a block's reconstruction visible to the workers that predict from it, and the layout of a worker's LDS slice.  Used by
 * intra_kernel.hip (the encode pass: source -> coefficients + reconstruction) and intra_recon_kernel.hip (the decode pass: coefficients ->
 * reconstruction).  Device code only; everything is internal linkage. */
#ifndef SVT_INTRA_CORE_H
#define SVT_INTRA_CORE_H
#include <hip/hip_runtime.h>
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

} // namespace
#endif
