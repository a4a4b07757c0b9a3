/*
 * mvrefs.hip -- the MV-reference derivation of batches of inter pictures (gfx950): grids -> the svt_mi_inter_ext records the inter
 * mode-info stage (modeinfo_inter.hip) takes, the candidate set of every block, and a count of leaves whose MVs contradict their mode.
 *
 * Replaces eb_vp9_find_mv_refs per block and reference frame (Source/Lib/VPX/vp9_mvref_common.c:20-197, called from
 * prepare_fast_loop_candidates, Codec/EbModeDecision.c:638-672).
 *
 * The derivation is a function of the grid (mvrefs_core.h): every candidate position lies above or left of its block, at most 3
 * units above or left of the block's origin.  So:
 *   svt_mvr_derive_kernel   one wave per (picture, SB), one lane per 8x8 unit in z-order.  The wave first stages the 11 x 11 window of
 *                           units that starts 3 above and 3 left of its SB into LDS, three dwords a unit (MV 0, MV 1, a meta word);
 *                           only the mode of a unit comes from elsewhere, the origin of its leaf, which may lie outside the window.
 *                           The lanes then run the walk from LDS alone and write their unit's records; the wave leaves its two sums
 *                           (contradicting leaves, inter leaves), or SVT_MODES_BAD_GRID, in the context's scratch
 *   svt_mvr_status_kernel   one workgroup per picture: the sums of the SBs -> d_status, in the shape of syn_scan_kernel (syntax_stage.h)
 * 1 452 bytes of LDS per wave: the 160 KB of a CU hold far more waves than its SIMDs take.  No atomics, and workgroups do not talk to
 * each other: the two passes are separate launches in stream order.
 */
#include <hip/hip_runtime.h>
#include "svt_ctx.h"
#include "mvrefs_core.h"
#include "wave_ops.h"

#define MVR_MAX_PICS 32
#define MVR_SCRATCH_SLOT 54

namespace {

struct mvr_pic_dev {
    svt_mvr_view      v;
    svt_mi_inter_ext *ext_out;
    svt_mvref_cand   *cand;
    uint32_t         *status, *part; /* part: [n_sb][2] */
};
struct mvr_batch_dev {
    mvr_pic_dev  pic[MVR_MAX_PICS];
    svt_tok_geom g;
    int32_t      n_sb, sb_cols;
};

__global__ __launch_bounds__(64) void svt_mvr_derive_kernel(const mvr_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_win[SVT_MVR_WIN_WORDS];
    const int sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const mvr_pic_dev &P = B->pic[pic];
    const svt_tok_geom g = B->g;
    const int sb_r = (sb / B->sb_cols) * 8, sb_c = (sb % B->sb_cols) * 8;
    for (int i = lane; i < SVT_MVR_WIN * SVT_MVR_WIN; i += 64) {
        const int     r = sb_r - 3 + i / SVT_MVR_WIN, c = sb_c - 3 + i % SVT_MVR_WIN;
        svt_mvr_entry e;
        e.mv0 = e.mv1 = e.meta = 0;
        if (r >= 0 && c >= 0 && r < g.mi_rows && c < g.mi_cols) e = svt_mvr_pack(&P.v, &g, r, c);
        s_win[3 * i] = e.mv0; s_win[3 * i + 1] = e.mv1; s_win[3 * i + 2] = e.meta;
    }
    int ur, uc;
    svt_tok_unit_of(lane, &ur, &uc);
    const int  r = sb_r + ur, c = sb_c + uc;
    const bool in = r < g.mi_rows && c < g.mi_cols;
    const bool bad = in && svt_mvr_check(&P.v, &g, r, c);
    const int  any_bad = wave_sum(bad ? 1 : 0);
    __syncthreads();
    int contradicts = 0, inter_leaf = 0;
    /* (an SB with a record the stage does not take is not analysed: its fields may be anything) */
    if (in && !any_bad) {
        const svt_mvr_unit_out o = svt_mvr_unit(&P.v, &g, s_win, ur + 3, uc + 3, r, c);
        const size_t           idx = (size_t)r * g.mi_stride + c;
        contradicts = o.contradicts;
        inter_leaf = o.inter_leaf;
        if (P.ext_out) {
            if (((uintptr_t)P.ext_out & 3) == 0) {
                uint32_t *d = (uint32_t *)(P.ext_out + idx);
                d[0] = o.e0; d[1] = o.e1; d[2] = o.e2;
            } else { /* (the record's own alignment is 2) */
                uint16_t *d = (uint16_t *)(P.ext_out + idx);
                d[0] = (uint16_t)o.e0; d[1] = (uint16_t)(o.e0 >> 16); d[2] = (uint16_t)o.e1; d[3] = (uint16_t)(o.e1 >> 16);
                d[4] = (uint16_t)o.e2; d[5] = (uint16_t)(o.e2 >> 16);
            }
        }
        if (P.cand) {
            if (((uintptr_t)P.cand & 15) == 0) {
                uint4 *d = (uint4 *)(P.cand + idx);
                d[0] = make_uint4(o.k0, o.k1, o.k2, o.k3);
                d[1] = make_uint4(o.k4, o.k5, o.k6, o.k7);
            } else {
                uint16_t *d = (uint16_t *)(P.cand + idx);
                d[0] = (uint16_t)o.k0; d[1] = (uint16_t)(o.k0 >> 16); d[2] = (uint16_t)o.k1; d[3] = (uint16_t)(o.k1 >> 16);
                d[4] = (uint16_t)o.k2; d[5] = (uint16_t)(o.k2 >> 16); d[6] = (uint16_t)o.k3; d[7] = (uint16_t)(o.k3 >> 16);
                d[8] = (uint16_t)o.k4; d[9] = (uint16_t)(o.k4 >> 16); d[10] = (uint16_t)o.k5; d[11] = (uint16_t)(o.k5 >> 16);
                d[12] = (uint16_t)o.k6; d[13] = (uint16_t)(o.k6 >> 16); d[14] = (uint16_t)o.k7; d[15] = (uint16_t)(o.k7 >> 16);
            }
        }
    }
    const int n_contra = wave_sum(contradicts), n_inter = wave_sum(inter_leaf);
    if (lane == 0) {
        P.part[2 * sb] = any_bad ? SVT_MODES_BAD_GRID : (uint32_t)n_contra;
        P.part[2 * sb + 1] = any_bad ? SVT_MODES_BAD_GRID : (uint32_t)n_inter;
    }
}

/* part[0 .. n_sb) -> status[0 .. 2): the sums, or SVT_MODES_BAD_GRID twice */
__global__ __launch_bounds__(256) void svt_mvr_status_kernel(const mvr_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_a[256], s_b[256];
    __shared__ uint32_t s_bad;
    const mvr_pic_dev &P = B->pic[blockIdx.x];
    const uint32_t    *a = P.part;
    const int n = B->n_sb, t = (int)threadIdx.x, per = (n + 255) / 256, b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    if (t == 0) s_bad = 0;
    __syncthreads();
    uint32_t sa = 0, sb = 0;
    bool     bad = false;
    for (int i = b; i < e; i++) { bad |= a[2 * i] == SVT_MODES_BAD_GRID; sa += a[2 * i]; sb += a[2 * i + 1]; }
    if (bad) s_bad = 1;
    s_a[t] = sa; s_b[t] = sb;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) { s_a[t] += s_a[t + d]; s_b[t] += s_b[t + d]; }
        __syncthreads();
    }
    if (t == 0) {
        P.status[0] = s_bad ? SVT_MODES_BAD_GRID : s_a[0];
        P.status[1] = s_bad ? SVT_MODES_BAD_GRID : s_b[0];
    }
}

} // namespace

extern "C" int32_t svt_hip_mvrefs_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_mvrefs_picture *pics, int32_t width, int32_t height, int32_t mi_stride) {
    if (!ctx || !pics || n_pics < 1 || n_pics > MVR_MAX_PICS || width < 8 || height < 8 || width > 8192 || height > 8192 || (width & 7) || (height & 7) ||
        mi_stride < (width >> 3))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "mvrefs: bad argument");
    for (int i = 0; i < n_pics; i++) {
        const svt_mvrefs_picture &p = pics[i];
        if (!p.d_lf_mi || !p.d_mc_mi || !p.d_ext || !p.d_status) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "mvrefs: null picture field");
        if (p.ref_mask & 0xF1) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "mvrefs: ref_mask names a reference frame outside 1 .. 3");
        if (p.d_ext_out == p.d_ext) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "mvrefs: d_ext_out must not alias d_ext");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    mvr_batch_dev hb;
    memset(&hb, 0, sizeof hb);
    hb.g.mi_stride = mi_stride; hb.g.mi_rows = height >> 3; hb.g.mi_cols = width >> 3; hb.g.w4 = width >> 2; hb.g.h4 = height >> 2;
    hb.sb_cols = (width + 63) >> 6;
    hb.n_sb = hb.sb_cols * ((height + 63) >> 6);
    uint32_t *part = (uint32_t *)svt_ctx_slot(ctx, MVR_SCRATCH_SLOT, sizeof(uint32_t) * 2 * (size_t)n_pics * (size_t)hb.n_sb);
    if (!part) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "mvrefs: scratch");
    for (int i = 0; i < n_pics; i++) {
        const svt_mvrefs_picture &p = pics[i];
        mvr_pic_dev &P = hb.pic[i];
        P.v.mi = p.d_lf_mi; P.v.mc = p.d_mc_mi; P.v.ext = p.d_ext;
        P.v.ref_mask = p.ref_mask; P.v.restrict_ref_mvs = p.restrict_ref_mvs != 0;
        for (int k = 0; k < 4; k++) P.v.sign_bias |= (uint8_t)((p.ref_frame_sign_bias[k] != 0) << k);
        P.ext_out = p.d_ext_out; P.cand = p.d_cand; P.status = p.d_status;
        P.part = part + 2 * (size_t)i * (size_t)hb.n_sb;
    }
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof hb, &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "mvrefs: descriptor buffers");
    HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
    memcpy(h, &hb, sizeof hb);
    HIP_TRY(hipMemcpyAsync(d, h, sizeof hb, hipMemcpyHostToDevice, ctx->stream));
    svt_ctx_stage_commit(ctx);
    const mvr_batch_dev *dB = (const mvr_batch_dev *)d;
    hipLaunchKernelGGL(svt_mvr_derive_kernel, dim3(n_pics * hb.n_sb), dim3(64), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_mvr_status_kernel, dim3(n_pics), dim3(256), 0, ctx->stream, dB);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->ev_stop, ctx->stream));
    ctx->timed = 1;
    return SVT_HIP_OK;
}
