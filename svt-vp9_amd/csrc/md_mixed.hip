/*
 * md_mixed.hip -- the mixed stand-in decision of an inter picture (gfx950): svt_md_mixed_unit (encdec_core.h, the same text as the host
 * form in host/encdec_host.c) for a batch of pictures, from the ME records and the open-loop intra search records of every SB.
 *
 * svt_md_mixed_kernel: like svt_md_default_kernel one wave per (picture, SB) and one lane per 8x8 unit.  Every lane walks the SB's whole
 * PU tree, so the 85 ME records (3 400 bytes) and the 84 OIS records of the blocks >= 8x8 (1 008 bytes) are staged in LDS once, with
 * coalesced dword loads.  The number of units written intra goes to the picture's counter once per wave: ballot, popcount, one atomicAdd
 * by lane 0.
 */
#include <hip/hip_runtime.h>
#include "svt_ctx.h"
#include "encdec_core.h"

#define MDM_MAX_PICS 32 /* pictures per launch (encdec.hip's ED_MAX_PICS: the stand-ins chunk a batch alike) */
#define MDM_OIS_USED 84 /* records of an SB the rule reads: 32x32, 16x16, 8x8 */

namespace {

struct mdm_pic_dev {
    const svt_me_pu_result *res;
    const svt_ois_block    *ois;
    svt_mc_mode_info       *mc_mi;
    svt_lf_mode_info       *lf_mi;
};
struct mdm_batch_dev {
    mdm_pic_dev pic[MDM_MAX_PICS];
    int32_t    *intra_units; /* counter of the launch's first picture */
    int32_t     n_sb, sb_cols, mi_rows, mi_cols, mi_stride;
    uint32_t    lambda, intra_penalty;
    int32_t     filter_level;
};

__global__ __launch_bounds__(64) void svt_md_mixed_zero_kernel(int32_t *__restrict__ counts, int n) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) counts[i] = 0;
}

__global__ __launch_bounds__(64) void svt_md_mixed_kernel(const mdm_batch_dev *__restrict__ B) {
    __shared__ svt_me_pu_result s_res[SVT_ME_PU_COUNT];
    __shared__ svt_ois_block    s_ois[MDM_OIS_USED];
    const int          sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const mdm_pic_dev &P = B->pic[pic];
    {
        const uint32_t *g = (const uint32_t *)(P.res + (size_t)sb * SVT_ME_PU_COUNT);
        uint32_t       *d = (uint32_t *)s_res;
        for (int i = lane; i < (int)(sizeof s_res / 4); i += 64) d[i] = g[i];
        g = (const uint32_t *)(P.ois + (size_t)sb * SVT_OIS_PER_SB);
        d = (uint32_t *)s_ois;
        for (int i = lane; i < (int)(sizeof s_ois / 4); i += 64) d[i] = g[i];
    }
    __syncthreads();
    const int r = lane >> 3, c = lane & 7, sr = sb / B->sb_cols, sc = sb % B->sb_cols, ur = sr * 8 + r, uc = sc * 8 + c;
    int       intra = 0;
    if (ur < B->mi_rows && uc < B->mi_cols) {
        svt_mc_mode_info mc;
        svt_lf_mode_info lf;
        intra = svt_md_mixed_unit(s_res, s_ois, r, c, sr, sc, B->mi_rows, B->mi_cols, B->lambda, B->intra_penalty, B->filter_level, &mc, &lf);
        P.mc_mi[ur * B->mi_stride + uc] = mc;
        P.lf_mi[ur * B->mi_stride + uc] = lf;
    }
    const int n = __popcll(__ballot(intra));
    if (lane == 0 && n) atomicAdd(&B->intra_units[pic], n);
}

} // namespace

extern "C" int32_t svt_hip_md_mixed_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_md_mixed_picture *pics, int32_t width, int32_t height, uint32_t lambda,
                                                 uint32_t intra_penalty, int32_t filter_level, int32_t mi_stride, int32_t *d_intra_units) {
    if (!ctx || n_pics < 1 || !pics || !d_intra_units || width < 8 || height < 8 || (width & 7) || (height & 7) || mi_stride < (width >> 3) || filter_level < 0 ||
        filter_level > 63)
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_mixed: bad argument");
    for (int i = 0; i < n_pics; i++) /* (every picture is looked at before anything is launched) */
        if (!pics[i].d_results || !pics[i].d_ois || !pics[i].d_mc_mi || !pics[i].d_lf_mi || ((uintptr_t)pics[i].d_results & 3) || ((uintptr_t)pics[i].d_ois & 3))
            return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_mixed: null or misaligned picture");
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(svt_md_mixed_zero_kernel, dim3((n_pics + 63) / 64), dim3(64), 0, ctx->stream, d_intra_units, n_pics);
    HIP_TRY(hipGetLastError());
    const int sb_cols = (width + 63) >> 6, n_sb = sb_cols * ((height + 63) >> 6);
    for (int first = 0; first < n_pics; first += MDM_MAX_PICS) {
        const int n = n_pics - first < MDM_MAX_PICS ? n_pics - first : MDM_MAX_PICS;
        void     *h = nullptr, *d = nullptr;
        if (svt_ctx_stage(ctx, sizeof(mdm_batch_dev), &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "md_mixed: descriptor buffers");
        mdm_batch_dev *hb = (mdm_batch_dev *)h;
        memset(hb, 0, sizeof *hb);
        hb->intra_units = d_intra_units + first; /* the count's index is the picture's index in the whole call */
        hb->n_sb = n_sb; hb->sb_cols = sb_cols; hb->mi_rows = height >> 3; hb->mi_cols = width >> 3; hb->mi_stride = mi_stride;
        hb->lambda = lambda; hb->intra_penalty = intra_penalty; hb->filter_level = filter_level;
        for (int i = 0; i < n; i++) {
            const svt_md_mixed_picture &p = pics[first + i];
            hb->pic[i].res = p.d_results; hb->pic[i].ois = p.d_ois; hb->pic[i].mc_mi = p.d_mc_mi; hb->pic[i].lf_mi = p.d_lf_mi;
        }
        HIP_TRY(svt_ctx_stage_send(ctx, sizeof(mdm_batch_dev)));
        hipLaunchKernelGGL(svt_md_mixed_kernel, dim3(n * n_sb), dim3(64), 0, ctx->stream, (const mdm_batch_dev *)d);
        HIP_TRY(hipGetLastError());
    }
    return SVT_HIP_OK;
}
