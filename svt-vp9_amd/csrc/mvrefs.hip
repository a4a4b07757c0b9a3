/*
 * mvrefs.hip -- the MV-reference derivation of batches of inter pictures (gfx950): grids -> the svt_mi_inter_ext records the inter
 * mode-info stage (modeinfo_inter.hip) takes, the candidate set of every block, and a count of leaves whose MVs contradict their mode.
 *
 * Replaces eb_vp9_find_mv_refs per block and reference frame (Source/Lib/VPX/vp9_mvref_common.c:20-197, called from
 * prepare_fast_loop_candidates, Codec/EbModeDecision.c:638-672).
 *
 * The derivation is a function of the grid (mvrefs_core.h): every candidate position lies above or left of its block, at most 3
 * units above or left of the block's origin.  So the stage is the window skeleton of mvrefs_stage.h as it stands, two launches:
 *   mvs_derive_kernel<mvr_stage>   one wave per (picture, SB) stages the 11 x 11 window of units that starts 3 above and 3 left of its SB
 *                                  into LDS, three dwords a unit (MV 0, MV 1, a meta word); only the mode of a unit comes from
 *                                  elsewhere, the origin of its leaf, which may lie outside the window.  The lanes then run the walk
 *                                  from LDS alone and write their unit's records; the wave leaves its two sums (contradicting leaves,
 *                                  inter leaves), or SVT_MODES_BAD_GRID, in the context's scratch
 *   mvs_status_kernel<mvr_stage>   one workgroup per picture: the sums of the SBs -> d_status[0 .. 2)
 */
#include "mvrefs_stage.h"

namespace {

struct mvr_stage {
    typedef svt_mvrefs_picture picture;
    struct pic_dev {
        svt_mvr_view      v;
        svt_mi_inter_ext *ext_out;
        svt_mvref_cand   *cand;
        uint32_t         *status, *part;
    };
    static constexpr int         N = 2, STATUS_WORDS = 2, PART_SLOT = SVT_SLOT_MVR_PART;
    static constexpr const char *NAME = "mvrefs";
    static __device__ __forceinline__ int also_refused(const pic_dev &, const svt_tok_geom *, int, int) { return 0; }
    static __device__ __forceinline__ void sums(const pic_dev &, const svt_tok_geom *, int, int, const svt_mvr_unit_out &o, int *s) {
        s[0] = o.contradicts;
        s[1] = o.inter_leaf;
    }
    static const char *fill(const picture &p, pic_dev &P) {
        if (const char *what = mvs_fill_common<mvr_stage>(p, P, p.d_ext, !p.d_ext)) return what;
        return p.d_ext_out == p.d_ext ? "d_ext_out must not alias d_ext" : nullptr;
    }
    static bool scratch(svt_hip_ctx *, mvs_batch_dev<mvr_stage> &, int) { return true; }
};

} // namespace

extern "C" int32_t svt_hip_mvrefs_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_mvrefs_picture *pics, int32_t width, int32_t height, int32_t mi_stride) {
    return mvs_batch_device<mvr_stage>(ctx, n_pics, pics, width, height, mi_stride, [&](const mvs_batch_dev<mvr_stage> *dB, int n_sb) {
        hipLaunchKernelGGL(mvs_derive_kernel<mvr_stage>, dim3(n_pics * n_sb), dim3(64), 0, ctx->stream, dB);
        hipLaunchKernelGGL(mvs_status_kernel<mvr_stage>, dim3(n_pics), dim3(256), 0, ctx->stream, dB);
    });
}
