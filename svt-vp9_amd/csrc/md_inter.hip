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
 *                           other two are never read)
 *   svt_mdi_derive_kernel   the same shape, over the scratch records: svt_mvr_check + svt_mdi_check, then the window of svt_mvr_pack (now
 *                           with the counter classes of the labels) and svt_mvr_unit, the text svt_hip_mvrefs_batch_device runs -> d_ext_out,
 *                           d_cand; the wave leaves its three sums, or SVT_MODES_BAD_GRID, in the context's scratch
 *   svt_mdi_status_kernel   one workgroup per picture: the sums of the SBs -> d_status[0 .. 4)
 * 1 452 bytes of LDS per wave.  No atomics.
 */
#include <hip/hip_runtime.h>
#include "svt_ctx.h"
#include "md_inter_core.h"
#include "wave_ops.h"

#define MDI_MAX_PICS 32
#define MDI_PART_SLOT 55
#define MDI_EXT_SLOT 56

namespace {

struct mdi_pic_dev {
    svt_mvr_view      v; /* v.ext: the scratch records */
    svt_mdi_frame     m;
    svt_mi_inter_ext *label, *ext_out;
    svt_mvref_cand   *cand;
    uint32_t         *status, *part; /* part: [n_sb][3] */
};
struct mdi_batch_dev {
    mdi_pic_dev  pic[MDI_MAX_PICS];
    svt_tok_geom g;
    int32_t      n_sb, sb_cols;
};

__global__ __launch_bounds__(64) void svt_mdi_label_kernel(const mdi_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_win[SVT_MVR_WIN_WORDS];
    const int sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const mdi_pic_dev &P = B->pic[pic];
    const svt_tok_geom g = B->g;
    const int sb_r = (sb / B->sb_cols) * 8, sb_c = (sb % B->sb_cols) * 8;
    for (int i = lane; i < SVT_MVR_WIN * SVT_MVR_WIN; i += 64) {
        const int     r = sb_r - 3 + i / SVT_MVR_WIN, c = sb_c - 3 + i % SVT_MVR_WIN;
        svt_mvr_entry e;
        e.mv0 = e.mv1 = e.meta = 0;
        if (r >= 0 && c >= 0 && r < g.mi_rows && c < g.mi_cols) e = svt_mdi_pack(&P.v, &P.m, &g, r, c);
        s_win[3 * i] = e.mv0; s_win[3 * i + 1] = e.mv1; s_win[3 * i + 2] = e.meta;
    }
    int ur, uc;
    svt_tok_unit_of(lane, &ur, &uc);
    const int r = sb_r + ur, c = sb_c + uc;
    __syncthreads();
    if (r < g.mi_rows && c < g.mi_cols) {
        uint32_t *d = (uint32_t *)(P.label + ((size_t)r * g.mi_stride + c)); /* (the scratch grid is the context's: 4-byte aligned) */
        d[2] = svt_mdi_label_unit(&P.v, &P.m, &g, s_win, ur + 3, uc + 3, r, c);
    }
}

__global__ __launch_bounds__(64) void svt_mdi_derive_kernel(const mdi_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_win[SVT_MVR_WIN_WORDS];
    const int sb = (int)blockIdx.x % B->n_sb, pic = (int)blockIdx.x / B->n_sb, lane = (int)threadIdx.x;
    const mdi_pic_dev &P = B->pic[pic];
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
    const bool bad = in && (P.m.bad || svt_mvr_check(&P.v, &g, r, c) || svt_mdi_check(&P.v, &P.m, &g, r, c));
    const int  any_bad = wave_sum(bad ? 1 : 0);
    __syncthreads();
    int inter_leaf = 0, newmv = 0, unfaithful = 0;
    /* (an SB with a record the stage does not take is not analysed: its fields may be anything) */
    if (in && !any_bad) {
        const svt_mvr_unit_out o = svt_mvr_unit(&P.v, &g, s_win, ur + 3, uc + 3, r, c);
        const size_t           idx = (size_t)r * g.mi_stride + c;
        inter_leaf = o.inter_leaf;
        svt_mdi_count(&P.v, &P.m, &g, r, c, &o, &newmv, &unfaithful);
        if (((uintptr_t)P.ext_out & 3) == 0) {
            uint32_t *d = (uint32_t *)(P.ext_out + idx);
            d[0] = o.e0; d[1] = o.e1; d[2] = o.e2;
        } else { /* (the record's own alignment is 2) */
            uint16_t *d = (uint16_t *)(P.ext_out + idx);
            d[0] = (uint16_t)o.e0; d[1] = (uint16_t)(o.e0 >> 16); d[2] = (uint16_t)o.e1; d[3] = (uint16_t)(o.e1 >> 16);
            d[4] = (uint16_t)o.e2; d[5] = (uint16_t)(o.e2 >> 16);
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
    const int n_inter = wave_sum(inter_leaf), n_new = wave_sum(newmv), n_unf = wave_sum(unfaithful);
    if (lane == 0) {
        P.part[3 * sb] = any_bad ? SVT_MODES_BAD_GRID : (uint32_t)n_inter;
        P.part[3 * sb + 1] = any_bad ? SVT_MODES_BAD_GRID : (uint32_t)n_new;
        P.part[3 * sb + 2] = any_bad ? SVT_MODES_BAD_GRID : (uint32_t)n_unf;
    }
}

/* part[0 .. n_sb) -> status[0 .. 4): the three sums and 0, or SVT_MODES_BAD_GRID four times */
__global__ __launch_bounds__(256) void svt_mdi_status_kernel(const mdi_batch_dev *__restrict__ B) {
    __shared__ uint32_t s_a[256], s_b[256], s_c[256];
    __shared__ uint32_t s_bad;
    const mdi_pic_dev &P = B->pic[blockIdx.x];
    const uint32_t    *a = P.part;
    const int n = B->n_sb, t = (int)threadIdx.x, per = (n + 255) / 256, b = t * per < n ? t * per : n, e = b + per < n ? b + per : n;
    if (t == 0) s_bad = 0;
    __syncthreads();
    uint32_t sa = 0, sb = 0, sc = 0;
    bool     bad = false;
    for (int i = b; i < e; i++) { bad |= a[3 * i] == SVT_MODES_BAD_GRID; sa += a[3 * i]; sb += a[3 * i + 1]; sc += a[3 * i + 2]; }
    if (bad) s_bad = 1;
    s_a[t] = sa; s_b[t] = sb; s_c[t] = sc;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) { s_a[t] += s_a[t + d]; s_b[t] += s_b[t + d]; s_c[t] += s_c[t + d]; }
        __syncthreads();
    }
    if (t < 4) P.status[t] = s_bad ? SVT_MODES_BAD_GRID : t == 0 ? s_a[0] : t == 1 ? s_b[0] : t == 2 ? s_c[0] : 0u;
}

} // namespace

extern "C" int32_t svt_hip_md_inter_modes_batch_device(svt_hip_ctx *ctx, int32_t n_pics, const svt_md_inter_picture *pics, int32_t width, int32_t height,
                                                       int32_t mi_stride) {
    if (!ctx || !pics || n_pics < 1 || n_pics > MDI_MAX_PICS || width < 8 || height < 8 || width > 8192 || height > 8192 || (width & 7) || (height & 7) ||
        mi_stride < (width >> 3))
        return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_inter: bad argument");
    for (int i = 0; i < n_pics; i++) {
        const svt_md_inter_picture &p = pics[i];
        if (!p.d_lf_mi || !p.d_mc_mi || !p.d_ext_out || !p.d_status) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_inter: null picture field");
        if (p.ref_mask & 0xF1) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_inter: ref_mask names a reference frame outside 1 .. 3");
        const svt_mdi_frame m = svt_mdi_frame_of(&p);
        if (svt_mii_bad_frame(&m.f)) return svt_set_error(SVT_HIP_ERR_BAD_PARAMETER, "md_inter: reference_mode above 2, or a compound reference outside 1 .. 3");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    mdi_batch_dev hb;
    memset(&hb, 0, sizeof hb);
    hb.g.mi_stride = mi_stride; hb.g.mi_rows = height >> 3; hb.g.mi_cols = width >> 3; hb.g.w4 = width >> 2; hb.g.h4 = height >> 2;
    hb.sb_cols = (width + 63) >> 6;
    hb.n_sb = hb.sb_cols * ((height + 63) >> 6);
    const size_t units = (size_t)hb.g.mi_rows * (size_t)mi_stride;
    uint32_t *part = (uint32_t *)svt_ctx_slot(ctx, MDI_PART_SLOT, sizeof(uint32_t) * 3 * (size_t)n_pics * (size_t)hb.n_sb);
    svt_mi_inter_ext *label = (svt_mi_inter_ext *)svt_ctx_slot(ctx, MDI_EXT_SLOT, sizeof(svt_mi_inter_ext) * (size_t)n_pics * units);
    if (!part || !label) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "md_inter: scratch");
    for (int i = 0; i < n_pics; i++) {
        const svt_md_inter_picture &p = pics[i];
        mdi_pic_dev &P = hb.pic[i];
        P.label = label + (size_t)i * units;
        P.v.mi = p.d_lf_mi; P.v.mc = p.d_mc_mi; P.v.ext = P.label;
        P.v.ref_mask = p.ref_mask; P.v.restrict_ref_mvs = p.restrict_ref_mvs != 0;
        for (int k = 0; k < 4; k++) P.v.sign_bias |= (uint8_t)((p.ref_frame_sign_bias[k] != 0) << k);
        P.m = svt_mdi_frame_of(&p);
        P.ext_out = p.d_ext_out; P.cand = p.d_cand; P.status = p.d_status;
        P.part = part + 3 * (size_t)i * (size_t)hb.n_sb;
    }
    void *h = nullptr, *d = nullptr;
    if (svt_ctx_stage(ctx, sizeof hb, &h, &d)) return svt_set_error(SVT_HIP_ERR_NO_RESOURCES, "md_inter: descriptor buffers");
    HIP_TRY(hipEventRecord(ctx->ev_start, ctx->stream));
    memcpy(h, &hb, sizeof hb);
    HIP_TRY(hipMemcpyAsync(d, h, sizeof hb, hipMemcpyHostToDevice, ctx->stream));
    svt_ctx_stage_commit(ctx);
    const mdi_batch_dev *dB = (const mdi_batch_dev *)d;
    hipLaunchKernelGGL(svt_mdi_label_kernel, dim3(n_pics * hb.n_sb), dim3(64), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_mdi_derive_kernel, dim3(n_pics * hb.n_sb), dim3(64), 0, ctx->stream, dB);
    hipLaunchKernelGGL(svt_mdi_status_kernel, dim3(n_pics), dim3(256), 0, ctx->stream, dB);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ctx->ev_stop, ctx->stream));
    ctx->timed = 1;
    return SVT_HIP_OK;
}
