/*
 * md_inter.hip -- inter mode labelling of batches of pictures (gfx950): the two grids the encode pass holds -> complete
 * svt_mi_inter_ext records (ref_frame everywhere; mode, ref_mv_* and mode_context at inter leaf origins), the candidate set of every
 * block, and the counts of inter, NEWMV and unfaithfully coded leaves.  The rule is csrc/md_inter_core.h's.
 *
 * A leaf's label needs its own candidates only, and those read the neighbours' ref_frame and MVs, never their modes; the mode context
 * needs the labels of the leaves above and left, whose origins may lie anywhere in the neighbouring SBs.  So two passes in stream order,
 * the second reading what the first wrote, and no workgroup ever waits for another:
 *   svt_mdi_label_kernel    one wave per (picture, SB), one lane per 8x8 unit in z-order.  The wave stages the 11 x 11 window of its SB in
 *                           LDS as mvrefs.hip does, packed from the grids alone (svt_mdi_pack); each lane writes ref_frame and -- at an
 *                           inter leaf's origin -- the label into its unit's record of the context's scratch grid (the third dword; the
 *                           other two are never read);
 * then the window skeleton of mvrefs_stage.h, the text svt_hip_mvrefs_batch_device runs, over the scratch records:
 *   mvs_derive_kernel<mdi_stage>   svt_mvr_check + svt_mdi_check, then the window of svt_mvr_pack (now with the counter classes of the
 *                                  labels) and svt_mvr_unit -> d_ext_out, d_cand; the wave leaves its three sums (inter, NEWMV and
 *                                  unfaithful leaves), or SVT_MODES_BAD_GRID, in the context's scratch
 *   mvs_status_kernel<mdi_stage>   one workgroup per picture: the sums of the SBs -> d_status[0 .. 4), the fourth word 0
 * 1 452 bytes of LDS per wave.  No atomics.
 */
#include "mvrefs_stage.h"
#include "md_inter_core.h"

namespace {

struct mdi_stage {
    typedef svt_md_inter_picture picture;
    struct pic_dev {
        svt_mvr_view      v; /* v.ext: the scratch records */
        svt_mdi_frame     m;
        svt_mi_inter_ext *label, *ext_out;
        svt_mvref_cand   *cand;
        uint32_t         *status, *part;
    };
    static constexpr int         N = 3, STATUS_WORDS = 4, PART_SLOT = SVT_SLOT_MDI_PART;
    static constexpr const char *NAME = "md_inter";
    static __device__ __forceinline__ int also_refused(const pic_dev &P, const svt_tok_geom *g, int r, int c) { return P.m.bad || svt_mdi_check(&P.v, &P.m, g, r, c); }
    static __device__ __forceinline__ void sums(const pic_dev &P, const svt_tok_geom *g, int r, int c, const svt_mvr_unit_out &o, int *s) {
        s[0] = o.inter_leaf;
        svt_mdi_count(&P.v, &P.m, g, r, c, &o, &s[1], &s[2]);
    }
    static const char *fill(const picture &p, pic_dev &P) {
        if (const char *what = mvs_fill_common<mdi_stage>(p, P, nullptr, !p.d_ext_out)) return what;
        P.m = svt_mdi_frame_of(&p);
        return svt_mii_bad_frame(&P.m.f) ? "reference_mode above 2, or a compound reference outside 1 .. 3" : nullptr;
    }
    static bool scratch(svt_hip_ctx *ctx, mvs_batch_dev<mdi_stage> &hb, int n_pics) {
        const size_t      units = (size_t)hb.g.mi_rows * (size_t)hb.g.mi_stride;
        svt_mi_inter_ext *label = (svt_mi_inter_ext *)svt_ctx_slot(ctx, SVT_SLOT_MDI_LABEL, sizeof(svt_mi_inter_ext) * (size_t)n_pics * units);
        for (int i = 0; label && i < n_pics; i++) hb.pic[i].v.ext = hb.pic[i].label = label + (size_t)i * units;
        return label != nullptr;
    }
};

__global__ __launch_bounds__(64) void svt_mdi_label_kernel(const mvs_batch_dev<mdi_stage> *__restrict__ B) {
    __shared__ uint32_t s_win[SVT_MVR_WIN_WORDS];
    const mvs_lane            w = mvs_lane_of(B->n_sb, B->sb_cols);
    const mdi_stage::pic_dev &P = B->pic[w.pic];
    const svt_tok_geom        g = B->g;
    mvs_stage_window(s_win, &g, w, [&](int r, int c) { return svt_mdi_pack(&P.v, &P.m, &g, r, c); });
    __syncthreads();
    if (w.r < g.mi_rows && w.c < g.mi_cols) {
        uint32_t *d = (uint32_t *)(P.label + ((size_t)w.r * g.mi_stride + w.c)); /* (the scratch grid is the context's: 4-byte aligned) */
        d[2] = svt_mdi_label_unit(&P.v, &P.m, &g, s_win, w.ur + 3, w.uc + 3, w.r, w.c);
    }
}

} // namespace

extern "C" int32_t svt_hip_md_inter_modes_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_md_inter_picture *pics, int32_t width, int32_t height,
                                                       int32_t mi_stride) {
    return mvs_batch_device<mdi_stage>(ctx, n_pics, pics, width, height, mi_stride, [&](const mvs_batch_dev<mdi_stage> *dB, int n_sb) {
        hipLaunchKernelGGL(svt_mdi_label_kernel, dim3(n_pics * n_sb), dim3(64), 0, ctx->stream, dB);
        hipLaunchKernelGGL(mvs_derive_kernel<mdi_stage>, dim3(n_pics * n_sb), dim3(64), 0, ctx->stream, dB);
        hipLaunchKernelGGL(mvs_status_kernel<mdi_stage>, dim3(n_pics), dim3(256), 0, ctx->stream, dB);
    });
}
